// top_k_kernels.hip — top-k (include/alpgpu.h, "top-k"): ORDER BY x [DESC] LIMIT k over a compressed column under a bitmap.
//
//   records      launch_minmax_masked into the scratch, unless the caller brought them: every vector's exact masked {min, max}
//   vector level the radix select below over {hi of the record's max (min), ~v} of the non-empty vectors: the threshold Tv, at or above which
//                lie exactly min(k, non-empty vectors) vectors.  They hold the whole result (the argument).
//   candidates   k_top_k_candidates<VB> (top_k_device.hpp): the kept vectors decoded in registers, {hi, ~index} of the selected values that are no
//                NaN and reach the value part of Tv (with fewer than k kept vectors: all of them) appended to an array of min(k, n_vectors) * 1024 pairs
//   element level the same select over the candidates: T*, at or above which lie exactly min(k, candidates) of them; k_top_k_filter appends those
//                to k staging slots
//   sort         k_top_k_sort<VB>: one workgroup, a bitonic sort in LDS, descending; it writes d_vals, d_idx and *d_count
//
// The radix select: 8-bit digits, most significant first, over hi's bytes and then the bytes of lo that differ between keys.  Per digit a histogram
// kernel (LDS bins per workgroup, only keys that match the digits settled so far, at most 256 integer atomics per workgroup into global bins, at most
// kTopKHistGrid workgroups) and a one-wavefront pick that walks the bins from the top and settles the digit and the remaining rank in TopKState.
// All counts live in device memory and every grid is fixed on the host; integer counts are exact and keys unique, so nothing depends on the order
// in which wavefronts arrive.  No workgroup waits for another.
#include "launch.hpp"
#include "top_k_device.hpp"

namespace alpgpu {

__device__ __forceinline__ void top_k_hist_take(uint32_t* s_bins, uint64_t hi, uint64_t lo, uint64_t thr_hi, uint64_t thr_lo, const TopKPass& p) {
	if ((((hi ^ thr_hi) & p.mask_hi) | ((lo ^ thr_lo) & p.mask_lo)) == 0ull) { atomicAdd(&s_bins[((p.in_lo ? lo : hi) >> p.shift) & 255ull], 1u); }
}
__device__ __forceinline__ void top_k_hist_flush(const uint32_t* s_bins, uint32_t* bins) {
	__syncthreads();
	const uint32_t n = s_bins[threadIdx.x];
	if (n != 0u) { atomicAdd(&bins[threadIdx.x], n); }
}

// the vector level's keys: one record per thread, grid-stride
template <int VB>
__global__ __launch_bounds__(kTopKHistThreads) void k_top_k_hist_vectors(const void* __restrict__ zones, uint64_t n_vectors, int largest, const TopKState* __restrict__ st, const TopKPass p,
                                                                         uint32_t* __restrict__ bins) {
	__shared__ uint32_t s_bins[256];
	s_bins[threadIdx.x] = 0u;
	__syncthreads();
	const uint64_t thr_hi = st->thr_hi, thr_lo = st->thr_lo;
	for (uint64_t v = static_cast<uint64_t>(blockIdx.x) * kTopKHistThreads + threadIdx.x; v < n_vectors; v += static_cast<uint64_t>(gridDim.x) * kTopKHistThreads) {
		uint64_t hi;
		if (top_k_record<VB>(zones, v, largest != 0, hi)) { top_k_hist_take(s_bins, hi, ~v, thr_hi, thr_lo, p); }
	}
	top_k_hist_flush(s_bins, bins);
}

// the element level's keys: the candidates, their number read here and clamped to the array
__global__ __launch_bounds__(kTopKHistThreads) void k_top_k_hist_candidates(const uint64_t* __restrict__ cand, uint32_t capacity, const TopKState* __restrict__ st, const TopKPass p,
                                                                            uint32_t* __restrict__ bins) {
	__shared__ uint32_t s_bins[256];
	s_bins[threadIdx.x] = 0u;
	__syncthreads();
	const uint64_t thr_hi = st->thr_hi, thr_lo = st->thr_lo;
	const uint32_t n      = st->n_items < capacity ? st->n_items : capacity;
	for (uint32_t i = blockIdx.x * kTopKHistThreads + threadIdx.x; i < n; i += gridDim.x * kTopKHistThreads) {
		const ulonglong2 c = reinterpret_cast<const ulonglong2*>(cand)[i];
		top_k_hist_take(s_bins, c.x, c.y, thr_hi, thr_lo, p);
	}
	top_k_hist_flush(s_bins, bins);
}

// One wavefront.  Lane l holds the bins of the digits 255 - 4 l .. 252 - 4 l, so an inclusive scan over the lanes counts the keys from the top.  The
// level's first pick starts from rank = count = min(k, keys there are); with fewer than k keys the threshold becomes the lowest key.  With none, count
// stays 0 and every later kernel of the call returns at once.
__global__ __launch_bounds__(64) void k_top_k_pick(const uint32_t* __restrict__ bins, TopKState* __restrict__ st, const TopKPass p) {
	const uint32_t lane = threadIdx.x;
	uint32_t       c[4];
#pragma unroll
	for (uint32_t j = 0; j < 4u; ++j) { c[j] = bins[255u - 4u * lane - j]; }
	const uint32_t own   = c[0] + c[1] + c[2] + c[3];
	const uint32_t incl  = wave_scan_add_u32(own);
	const uint32_t total = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(incl), 63));
	uint64_t       thr_hi = st->thr_hi, thr_lo = st->thr_lo;
	uint32_t       rank = st->rank, count = st->count;
	if (p.first) {
		count  = total < p.k ? total : p.k;
		rank   = count;
		thr_hi = 0ull;
		thr_lo = p.fill_lo;
		if (count == 0u) {
			if (lane == 0u) {
				st->thr_hi = thr_hi;
				st->thr_lo = thr_lo;
				st->rank   = 0u;
				st->count  = 0u;
			}
			return;
		}
	}
	if (count == 0u) { return; }
	uint32_t above = incl - own; // keys whose digit lies above this lane's four
	if (above < rank && rank <= incl) { // exactly one lane
		uint32_t digit = 0, left = rank;
		bool     found = false;
#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) {
			if (!found && rank <= above + c[j]) {
				digit = 255u - 4u * lane - j;
				left  = rank - above;
				found = true;
			}
			above += c[j];
		}
		const uint64_t d = static_cast<uint64_t>(digit) << p.shift;
		st->thr_hi       = p.in_lo ? thr_hi : (thr_hi | d);
		st->thr_lo       = p.in_lo ? (thr_lo | d) : thr_lo;
		st->rank         = left;
		st->count        = count;
	}
}

// the candidates at or above T* into the staging slots: one atomic add per wavefront and trip, the slot of a lane from mbcnt, clamped to k
__global__ __launch_bounds__(kTopKHistThreads) void k_top_k_filter(const uint64_t* __restrict__ cand, uint32_t capacity, TopKState* __restrict__ st, uint64_t* __restrict__ stage, uint32_t k) {
	const uint32_t lane = threadIdx.x & 63u;
	if (st->count == 0u) { return; }
	const uint64_t thr_hi = st->thr_hi, thr_lo = st->thr_lo;
	const uint32_t n      = st->n_items < capacity ? st->n_items : capacity;
	const uint32_t step   = gridDim.x * kTopKHistThreads;
	for (uint32_t i0 = blockIdx.x * kTopKHistThreads + (threadIdx.x & ~63u); i0 < n; i0 += step) { // (i0: wave-uniform)
		const uint32_t i = i0 + lane;
		ulonglong2     c = make_ulonglong2(0ull, 0ull);
		if (i < n) { c = reinterpret_cast<const ulonglong2*>(cand)[i]; }
		const uint64_t take = ballot64(i < n && top_k_at_or_above(c.x, c.y, thr_hi, thr_lo));
		if (take == 0ull) { continue; }
		uint32_t base = 0;
		if (lane == 0u) { base = atomicAdd(&st->n_stage, static_cast<uint32_t>(__builtin_popcountll(take))); }
		base                = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(base)));
		const uint32_t slot = mbcnt64(take, base);
		if (((take >> lane) & 1ull) && slot < k) { reinterpret_cast<ulonglong2*>(stage)[slot] = c; }
	}
}

__device__ __forceinline__ bool top_k_below(const ulonglong2& a, const ulonglong2& b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }

// One workgroup of n_sort threads (a power of two, >= 64 and >= k): the staged keys, padded with {0, 0} (below every key: no index is all ones),
// sorted descending by a bitonic network in LDS; then the values out of the keys, the indices, and the count.
template <int VB>
__global__ __launch_bounds__(kTopKSortMax) void k_top_k_sort(const uint64_t* __restrict__ stage, const TopKState* __restrict__ st, uint32_t k, int largest, void* __restrict__ d_vals,
                                                             int64_t* __restrict__ d_idx, uint64_t* __restrict__ d_count) {
	__shared__ ulonglong2 s_key[kTopKSortMax];
	const uint32_t        t = threadIdx.x, n_sort = blockDim.x;
	uint32_t              m = st->count < st->n_stage ? st->count : st->n_stage;
	m                       = m < k ? m : k;
	s_key[t]                = t < m ? reinterpret_cast<const ulonglong2*>(stage)[t] : make_ulonglong2(0ull, 0ull);
	for (uint32_t size = 2u; size <= n_sort; size <<= 1) {
		for (uint32_t stride = size >> 1; stride > 0u; stride >>= 1) {
			__syncthreads();
			const uint32_t partner = t ^ stride;
			if (partner > t) {
				const ulonglong2 a = s_key[t], b = s_key[partner];
				if ((t & size) == 0u ? top_k_below(a, b) : top_k_below(b, a)) {
					s_key[t]       = b;
					s_key[partner] = a;
				}
			}
		}
	}
	__syncthreads();
	if (t < m) {
		const ulonglong2 key  = s_key[t];
		const uint64_t   bits = top_k_bits_of_hi<VB>(key.x, largest != 0);
		if constexpr (VB == 8) { static_cast<uint64_t*>(d_vals)[t] = bits; } else { static_cast<uint32_t*>(d_vals)[t] = static_cast<uint32_t>(bits); }
		if (d_idx != nullptr) { d_idx[t] = static_cast<int64_t>(~key.y); }
	}
	if (t == 0u) { *d_count = m; }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------------
// bytes of n - 1: the bytes of an index below n that can be non-zero
static uint32_t index_bytes(uint64_t n) {
	uint32_t b = 0;
	for (uint64_t top = n > 0 ? n - 1 : 0; top != 0; top >>= 8) { ++b; }
	return b;
}

// the passes of one level: hi's value_bytes digits, then lo's idx_bytes digits, most significant first
static TopKPass top_k_pass(uint32_t d, int value_bytes, uint32_t idx_bytes, uint32_t k) {
	const uint64_t idx_mask = idx_bytes >= 8u ? ~0ull : (1ull << (8u * idx_bytes)) - 1ull;
	TopKPass       p {};
	p.first   = d == 0u;
	p.k       = k;
	p.fill_lo = ~idx_mask;
	if (d < static_cast<uint32_t>(value_bytes)) {
		p.in_lo   = 0u;
		p.shift   = 8u * (static_cast<uint32_t>(value_bytes) - 1u - d);
		p.mask_hi = p.shift + 8u >= 64u ? 0ull : ~0ull << (p.shift + 8u);
		p.mask_lo = 0ull;
	} else {
		p.in_lo   = 1u;
		p.shift   = 8u * (idx_bytes - 1u - (d - static_cast<uint32_t>(value_bytes)));
		p.mask_hi = ~0ull;
		p.mask_lo = (p.shift + 8u >= 64u ? 0ull : ~0ull << (p.shift + 8u)) & idx_mask;
	}
	return p;
}

static unsigned hist_grid(uint64_t n) {
	const uint64_t wgs = (n + kTopKHistThreads - 1) / kTopKHistThreads;
	return wgs < 1 ? 1u : wgs < kTopKHistGrid ? static_cast<unsigned>(wgs) : kTopKHistGrid;
}

template <int VB>
static int top_k(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, const void* d_records, uint32_t k, int largest, void* d_vals, int64_t* d_idx, uint64_t* d_count,
                 void* d_scratch) {
	TopKLayout L;
	if (!top_k_layout(col->n_vectors, k, L)) { return ALPGPU_ERR_INVALID; }
	uint8_t* const   base  = static_cast<uint8_t*>(d_scratch);
	uint32_t* const  bins  = reinterpret_cast<uint32_t*>(base + L.bins);
	TopKState* const state = reinterpret_cast<TopKState*>(base + L.state);
	uint64_t* const  cand  = reinterpret_cast<uint64_t*>(base + L.cand);
	uint64_t* const  stage = reinterpret_cast<uint64_t*>(base + L.stage);
	const uint64_t   nv    = col->n_vectors;
	const uint32_t   cap   = static_cast<uint32_t>(L.cand_capacity);

	// the bins of every pass and both states, zeroed up front (they are contiguous)
	if (hipMemsetAsync(bins, 0, L.total - L.bins, stream) != hipSuccess) { return ALPGPU_ERR_HIP; }
	// 1. the records
	const void* zones = d_records;
	if (zones == nullptr) {
		const int rc = launch_minmax_masked(stream, col, d_mask, base + L.records, nullptr, VB);
		if (rc != ALPGPU_OK) { return rc; }
		zones = base + L.records;
	}
	// 2. the vector level
	const uint32_t passes_v = VB + index_bytes(nv);
	for (uint32_t d = 0; d < passes_v; ++d) {
		const TopKPass p = top_k_pass(d, VB, index_bytes(nv), k);
		hipLaunchKernelGGL((k_top_k_hist_vectors<VB>), dim3(hist_grid(nv)), dim3(kTopKHistThreads), 0, stream, zones, nv, largest, state, p, bins + 256u * d);
		hipLaunchKernelGGL(k_top_k_pick, dim3(1), dim3(64), 0, stream, bins + 256u * d, state, p);
	}
	if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	// 3. the candidates
	{
		TopKCandArgs g {};
		g.n_vectors = nv;
		g.mask      = d_mask;
		g.zones     = zones;
		g.vec       = state;
		g.elem      = state + 1;
		g.cand      = cand;
		g.capacity  = cap;
		g.k         = k;
		g.largest   = largest;
		const ColumnStreams c = column_streams(col);
		const int rc = launch_vectors(nv, kSelWaves, [&](dim3 grid, uint64_t off) {
			g.wg_off = off;
			hipLaunchKernelGGL((k_top_k_candidates<VB>), grid, dim3(kSelThreads), 0, stream, c, g);
		});
		if (rc != ALPGPU_OK) { return rc; }
	}
	// 4. the element level
	const uint32_t idx_b    = index_bytes(nv << 10);
	const uint32_t passes_e = VB + idx_b;
	uint32_t* const bins_e  = bins + 256u * kTopKMaxPasses;
	for (uint32_t d = 0; d < passes_e; ++d) {
		const TopKPass p = top_k_pass(d, VB, idx_b, k);
		hipLaunchKernelGGL(k_top_k_hist_candidates, dim3(hist_grid(cap)), dim3(kTopKHistThreads), 0, stream, cand, cap, state + 1, p, bins_e + 256u * d);
		hipLaunchKernelGGL(k_top_k_pick, dim3(1), dim3(64), 0, stream, bins_e + 256u * d, state + 1, p);
	}
	hipLaunchKernelGGL(k_top_k_filter, dim3(hist_grid(cap)), dim3(kTopKHistThreads), 0, stream, cand, cap, state + 1, stage, k);
	// 5. the sort and the result
	uint32_t n_sort = 64u;
	while (n_sort < k) { n_sort <<= 1; }
	hipLaunchKernelGGL((k_top_k_sort<VB>), dim3(1), dim3(n_sort), 0, stream, stage, state + 1, k, largest, d_vals, d_idx, d_count);
	return hipGetLastError() == hipSuccess ? ALPGPU_OK : ALPGPU_ERR_HIP;
}

int launch_top_k(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, const void* d_records, uint32_t k, int largest, void* d_vals, int64_t* d_idx, uint64_t* d_count,
                 void* d_scratch, int value_bytes) {
	return value_bytes == 8 ? top_k<8>(stream, col, d_mask, d_records, k, largest, d_vals, d_idx, d_count, d_scratch)
	                        : top_k<4>(stream, col, d_mask, d_records, k, largest, d_vals, d_idx, d_count, d_scratch);
}

} // namespace alpgpu
