// quantile_kernels.hip — quantiles (include/alpgpu.h, "quantiles"): the r-th smallest selected values of a compressed column, by an exact radix select
// over okey(x) with 8-bit digits, most significant first.  The launch sequence, fixed on the host:
//
//   memset            the state and the bins of every pass
//   k_quantile_popcount   the bitmap's set bits: if they fit the candidate capacity, pass 0 itself compacts and the call is ONE decode
//   per digit d:
//     k_quantile_wide<VB>   persistent workgroups of kQWaves wavefronts over the column's vectors (the shape of persistent_scan.hpp: one barrier for the LDS
//                           set-up, then v = wave id, wave id + waves, ...); per vector quantile_device.hpp's q_vector.  32 slots x 256 bins of LDS
//                           and 2 KiB of staged candidate keys per wavefront; the bins are
//                           flushed into the pass's 64-bit global bins at the end (and every flush_every trips, so that no 32-bit bin overflows).
//                           Returns at once when the state says "narrow".
//     k_quantile_narrow     (d >= 1) the same histogram over the candidate keys; returns at once unless the state says "narrow"
//     k_quantile_pick       one workgroup: pass 0 sets N and resolves the ranks; then per rank the digit, the remaining rank and the matching count
//                           from its slot's bins, the distinct prefixes as the next pass's slots, and the next pass's mode
//   k_quantile_finish<VB> the value bits out of the settled prefixes, d_ranks and *d_count
//
// All counts live in device memory, every grid is fixed on the host, only integer atomics are used and no workgroup waits for another.
//
// The flush, sized before it was written (it accumulates across workgroups): a workgroup adds at most 32 x 256 64-bit
// words, 64 KiB, per pass, and only its non-zero bins.  With 3 workgroups on each of 256 CUs that is at most 48 MiB of atomic adds per pass; at the
// chip-wide atomic rate of about 1.3 TB/s, 40 us beside a decode pass of about 2 ms.  So the bins are added straight into the global bins; no
// per-workgroup slabs.
#include "launch.hpp"
#include "quantile_device.hpp"

namespace alpgpu {

__global__ __launch_bounds__(256) void k_quantile_popcount(const uint64_t* __restrict__ mask, uint64_t n_words, QState* __restrict__ st) {
	uint32_t n = 0; // (a thread sees at most 2^36 / gridDim.x / 256 words: the grid is sized so that the wavefront's sum stays below 2^32)
	for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x; i < n_words; i += static_cast<uint64_t>(gridDim.x) * 256u) {
		n += static_cast<uint32_t>(__builtin_popcountll(mask[i]));
	}
	const uint32_t incl = wave_scan_add_u32(n);
	if ((threadIdx.x & 63u) == 63u && incl != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(&st->set_bits), static_cast<unsigned long long>(incl)); }
}

// the LDS set-up of both histogram kernels: the live slots' bins zeroed, the slot prefixes staged (pass 0: one slot, the empty prefix)
__device__ __forceinline__ uint32_t q_stage(const QState* st, uint32_t pass, uint32_t* s_bins, uint64_t* s_pfx) {
	uint32_t n_slots = pass == 0u ? 1u : st->n_slots;
	n_slots          = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(n_slots < 1u ? 1u : n_slots < kQSlots ? n_slots : kQSlots)));
	bins_zero<kQThreads>(s_bins, 256u * n_slots);
	if (threadIdx.x < kQSlots) { s_pfx[threadIdx.x] = pass > 0u && threadIdx.x < n_slots ? st->slot_prefix[threadIdx.x] : (threadIdx.x == 0u ? 0ull : ~0ull); }
	__syncthreads();
	return n_slots;
}

// the workgroup's loop, compiled twice: a compacting pass stages and appends the candidates, a plain one carries none of that
template <int VB, bool COMPACT>
__device__ __forceinline__ void q_wide_loop(const ColumnStreams& c, const QWideArgs& g, uint32_t wave, uint32_t lane, uint32_t n_slots, uint32_t* s_bins, const uint64_t* s_pfx,
                                            uint64_t (&s_exc)[kQWaves][16], uint64_t* s_keys, uint32_t& zero_skips, uint32_t& zone_skips) {
	// every wavefront of the workgroup makes the same number of trips (the last may find no vector), so that the flush's barriers are met by all
	const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * kQWaves;
	uint32_t       trips = 0, fill = 0; // fill: keys the wavefront has staged for the candidates
	for (uint64_t k0 = static_cast<uint64_t>(blockIdx.x) * kQWaves; k0 < g.n_vectors; k0 += n_waves) {
		const uint64_t v = k0 + wave;
		if (v < g.n_vectors) {
			const uint32_t did = q_vector<VB, COMPACT>(c, g, v, wave, lane, n_slots, s_bins, s_pfx, s_exc, s_keys, fill);
			zero_skips += did == kQSkipZero ? 1u : 0u;
			zone_skips += did == kQSkipZone ? 1u : 0u;
		}
		if (++trips == g.flush_every) {
			trips = 0;
			bins_flush<kQThreads>(s_bins, 256u * n_slots, g.bins);
			__syncthreads();
			bins_zero<kQThreads>(s_bins, 256u * n_slots);
			__syncthreads();
		}
	}
	if (COMPACT) { q_append(g, s_keys, fill, lane); }
}

// (6 wavefronts per SIMD are 3 workgroups per CU, what their LDS admits: the compiler is held to the 80 registers that takes)
template <int VB>
__global__ __launch_bounds__(kQThreads) __attribute__((amdgpu_waves_per_eu(6))) void k_quantile_wide(const ColumnStreams c, const QWideArgs g) {
	__shared__ uint32_t s_bins[kQSlots * 256u];
	__shared__ uint64_t s_pfx[kQSlots];
	__shared__ uint64_t s_exc[kQWaves][16]; // per wavefront: bit p = value p is an exception
	__shared__ uint64_t s_keys[kQWaves][kQStageKeys]; // per wavefront: the candidate keys staged for the next append

	const uint32_t mode = q_mode(g.st, g.pass, g.capacity);
	if (mode == kQNarrow || (g.pass > 0u && g.st->n == 0ull)) { return; } // (the same for every workgroup of the launch)
	const uint32_t wave    = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane    = threadIdx.x & 63u;
	const uint32_t n_slots = q_stage(g.st, g.pass, s_bins, s_pfx);

	uint32_t zero_skips = 0, zone_skips = 0;
	if (mode == kQCompact) {
		q_wide_loop<VB, true>(c, g, wave, lane, n_slots, s_bins, s_pfx, s_exc, s_keys[wave], zero_skips, zone_skips);
	} else {
		q_wide_loop<VB, false>(c, g, wave, lane, n_slots, s_bins, s_pfx, s_exc, s_keys[wave], zero_skips, zone_skips);
	}
	bins_flush<kQThreads>(s_bins, 256u * n_slots, g.bins);
	if (lane == 0u) { // the trace: one add per wavefront and counter
		if (g.pass == 0u && zero_skips != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(&g.st->zero_skips), static_cast<unsigned long long>(zero_skips)); }
		if (zone_skips != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(&g.st->zone_skips[g.pass & 7u]), static_cast<unsigned long long>(zone_skips)); }
	}
}

struct QNarrowArgs {
	const QState*   st;
	const uint64_t* cand;
	uint64_t*       bins; // of this pass
	uint64_t        capacity;
	uint64_t        mask_hi;
	uint32_t        shift;
	uint32_t        pass; // >= 1
};

// the candidates, their number read here and clamped to the array; a workgroup with no candidate returns before it touches its LDS
__global__ __launch_bounds__(kQThreads) void k_quantile_narrow(const QNarrowArgs g) {
	__shared__ uint32_t s_bins[kQSlots * 256u];
	__shared__ uint64_t s_pfx[kQSlots];
	if (g.st->mode != kQNarrow || g.st->n == 0ull) { return; }
	const uint64_t n = g.st->n_cand < g.capacity ? g.st->n_cand : g.capacity;
	if (static_cast<uint64_t>(blockIdx.x) * kQThreads >= n) { return; }
	const uint32_t n_slots = q_stage(g.st, g.pass, s_bins, s_pfx);
	for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kQThreads + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * kQThreads) {
		const uint64_t key = g.cand[i];
		uint32_t       slot;
		if (q_find_slot(s_pfx, n_slots, key & g.mask_hi, slot)) { atomicAdd(&s_bins[256u * slot + static_cast<uint32_t>((key >> g.shift) & 255ull)], 1u); }
	}
	bins_flush<kQThreads>(s_bins, 256u * n_slots, g.bins);
}

__device__ __forceinline__ uint64_t wave_scan_add_u64(uint64_t x, uint32_t lane) {
	for (uint32_t d = 1; d < 64u; d <<= 1) {
		const uint64_t y = __shfl_up(static_cast<unsigned long long>(x), d, 64);
		x += lane >= d ? y : 0ull;
	}
	return x;
}

struct QPickArgs {
	uint64_t capacity;
	uint32_t pass, shift;
	uint32_t vb, pad;
	QRequest req;
};

// the rank of entry r once N (> 0) is known.  A quantile's: min(N - 1, floor(q * (N - 1))), one IEEE double multiplication, not fused, then floor;
// entry 2 j is that rank, entry 2 j + 1 its upper neighbour
__device__ __forceinline__ uint64_t q_resolve(const QRequest& req, uint32_t r, uint64_t n) {
	const uint64_t last = n - 1ull;
	if (req.quantile) {
		const double   pos = __dmul_rn(req.q[(r >> 1) & (kQSlots / 2 - 1u)], static_cast<double>(last));
		uint64_t       at  = static_cast<uint64_t>(floor(pos));
		at                 = at < last ? at : last;
		return (r & 1u) && at < last ? at + 1ull : at;
	}
	const uint64_t at = req.ranks[r] < last ? req.ranks[r] : last;
	return req.from_top ? last - at : at;
}

// One workgroup of 16 wavefronts, a rank per wavefront and trip.  Lane l holds the bins of the digits 4 l .. 4 l + 3 of the rank's slot, so an inclusive
// scan over the lanes counts the keys from the bottom; the lane whose four bins hold the rank settles the digit, the remaining rank and the count.
// A rank at or behind the slot's total, which happens only with records that lie, clamps to the last non-empty bin (none: digit 0, count 0).
// Then wavefront 0 rebuilds the slots: the distinct new prefixes, ascending, whatever the order of the ranks.
__global__ __launch_bounds__(1024) void k_quantile_pick(QState* __restrict__ st, const uint64_t* __restrict__ bins, const QPickArgs p) {
	__shared__ uint64_t s_prefix[kQSlots], s_rem[kQSlots], s_cnt[kQSlots], s_res[kQSlots];
	__shared__ uint64_t s_n;
	const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
	const uint32_t mode = q_mode(st, p.pass, p.capacity);
	const uint32_t n_r  = p.req.n < kQSlots ? p.req.n : kQSlots;
	if (p.pass > 0u && st->n == 0ull) { return; }
	for (uint32_t r = wave; r < n_r; r += 16u) {
		const uint32_t  slot = p.pass == 0u ? 0u : (st->rank[r].slot < kQSlots ? st->rank[r].slot : kQSlots - 1u);
		const uint64_t* b    = bins + 256u * slot + 4u * lane;
		const uint64_t  c[4] = {b[0], b[1], b[2], b[3]};
		const uint64_t  own  = c[0] + c[1] + c[2] + c[3];
		const uint64_t  incl = wave_scan_add_u64(own, lane);
		const uint64_t  total = __shfl(static_cast<unsigned long long>(incl), 63, 64);
		uint64_t        rem, prefix;
		if (p.pass == 0u) {
			if (r == 0u && lane == 0u) { s_n = total; }
			if (total == 0ull) { continue; } // N == 0: nothing to settle (the same for every rank)
			rem    = q_resolve(p.req, r, total);
			prefix = 0ull;
			if (lane == 0u) { s_res[r] = rem; }
		} else {
			rem    = st->rank[r].rem;
			prefix = st->rank[r].prefix;
		}
		if (total == 0ull) {
			if (lane == 0u) { s_prefix[r] = prefix, s_rem[r] = 0ull, s_cnt[r] = 0ull; }
			continue;
		}
		rem            = rem < total ? rem : total - 1ull;
		uint64_t below = incl - own; // keys whose digit lies below this lane's four
		if (below <= rem && rem < incl) { // exactly one lane
			uint32_t digit = 0;
			uint64_t left = 0, cnt = 0;
			bool     found = false;
#pragma unroll
			for (uint32_t j = 0; j < 4u; ++j) {
				if (!found && rem < below + c[j]) {
					digit = 4u * lane + j;
					left  = rem - below;
					cnt   = c[j];
					found = true;
				}
				below += c[j];
			}
			s_prefix[r] = prefix | (static_cast<uint64_t>(digit) << p.shift);
			s_rem[r]    = left;
			s_cnt[r]    = cnt;
		}
	}
	__syncthreads();
	if (wave != 0u) { return; }
	if (p.pass == 0u) {
		if (lane == 0u) { st->n = s_n; }
		if (s_n == 0ull) { return; }
	}
	// the slots of the next pass: entry i is the FIRST of its prefix if no earlier entry has it; its slot is the number of distinct prefixes below it
	const bool     live   = lane < n_r;
	const uint64_t mine   = live ? s_prefix[lane & (kQSlots - 1u)] : 0ull;
	bool           first  = live;
	for (uint32_t j = 0; j < n_r; ++j) { first = first && !(j < lane && s_prefix[j] == mine); }
	const uint64_t firsts = ballot64(first);
	uint32_t       slot   = 0;
	uint64_t       sum    = 0; // the keys that match some slot: the candidates a compacting pass would append
	for (uint32_t j = 0; j < n_r; ++j) {
		const bool f = (firsts >> j) & 1ull;
		slot += f && s_prefix[j] < mine ? 1u : 0u;
		sum += f ? s_cnt[j] : 0ull;
	}
	if (live) {
		QRank e;
		e.prefix = mine, e.rem = s_rem[lane], e.cnt = s_cnt[lane], e.slot = slot, e.pad = 0u;
		st->rank[lane] = e;
		if (first) { st->slot_prefix[slot] = mine; }
		if (p.pass == 0u) { st->resolved[lane] = s_res[lane]; }
	}
	if (lane == 0u) {
		st->n_slots = static_cast<uint32_t>(__builtin_popcountll(firsts));
		st->mode    = mode != kQPlain ? kQNarrow : (sum <= p.capacity ? kQCompact : kQPlain);
		if (mode == kQCompact) { st->compact_p1 = p.pass + 1u; }
	}
}

struct QFinishArgs {
	void*     d_vals;
	uint64_t* d_ranks; // nullable
	uint64_t* d_count;
	uint32_t  n, quantile;
	uint32_t  wide_grid, waves_per_wg; // the trace
};

template <int VB>
__global__ __launch_bounds__(64) void k_quantile_finish(QState* __restrict__ st, const QFinishArgs f) {
	const uint32_t t = threadIdx.x;
	const uint64_t n = st->n;
	if (t == 0u) {
		*f.d_count       = n;
		st->wide_grid    = f.wide_grid;
		st->waves_per_wg = f.waves_per_wg;
		st->vb           = VB;
	}
	if (n == 0ull || t >= f.n || t >= kQSlots) { return; }
	const uint64_t bits = top_k_bits_of_hi<VB>(st->rank[t].prefix, true);
	if constexpr (VB == 8) { static_cast<uint64_t*>(f.d_vals)[t] = bits; } else { static_cast<uint32_t*>(f.d_vals)[t] = static_cast<uint32_t>(bits); }
	if (f.quantile && f.d_ranks != nullptr && (t & 1u) == 0u) { f.d_ranks[t >> 1] = st->resolved[t]; }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------------------
template <int VB>
static int quantile(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, const void* d_zones, const QRequest& req, void* d_vals, uint64_t* d_ranks, uint64_t* d_count,
                    void* d_scratch, int n_cus, const alpgpu_quantile_tuning& tune) {
	QuantileLayout L;
	if (!quantile_layout(col->n_vectors, L)) { return ALPGPU_ERR_INVALID; }
	uint8_t* const  base  = static_cast<uint8_t*>(d_scratch);
	QState* const   state = reinterpret_cast<QState*>(base + L.state);
	uint64_t* const bins  = reinterpret_cast<uint64_t*>(base + L.bins);
	uint64_t* const cand  = reinterpret_cast<uint64_t*>(base + L.cand);
	const uint64_t  nv    = col->n_vectors;
	const uint64_t  cap   = tune.capacity != 0 && tune.capacity < L.capacity ? tune.capacity : L.capacity; // (may only be lowered: the array has L.capacity keys)
	static_assert(sizeof(QState) <= kQuantileStateBytes, "the state fits its part of the scratch");

	if (hipMemsetAsync(base + L.state, 0, L.cand - L.state, stream) != hipSuccess) { return ALPGPU_ERR_HIP; } // the state and the bins of every pass (contiguous)
	{
		const uint64_t n_words = 16ull * nv;
		const uint64_t wgs     = (n_words + 2047ull) / 2048ull;
		// at most 2^36 words: with 1024 workgroups a wavefront sums at most 2^36 / 4096 * 64 = 2^30 bits
		hipLaunchKernelGGL(k_quantile_popcount, dim3(static_cast<unsigned>(wgs < 1024ull ? wgs : 1024ull)), dim3(256), 0, stream, d_mask, n_words, state);
	}
	const unsigned grid_wide   = persistent_grid(nv, kQWaves, n_cus, kQWgPerCu, tune.max_workgroups); // (the tuning's max_workgroups lowers what counts as resident)
	const uint64_t wg_narrow   = (cap + kQThreads - 1) / kQThreads;
	const unsigned grid_narrow = static_cast<unsigned>(wg_narrow < 256ull ? wg_narrow : 256ull);
	const ColumnStreams c = column_streams(col);
	const uint64_t all = VB == 8 ? ~0ull : 0xFFFFFFFFull;
	for (uint32_t d = 0; d < static_cast<uint32_t>(VB); ++d) {
		const uint32_t shift   = 8u * (static_cast<uint32_t>(VB) - 1u - d);
		const uint64_t mask_hi = shift + 8u >= 64u ? 0ull : (~0ull << (shift + 8u)) & all;
		uint64_t* const pass_bins = bins + static_cast<uint64_t>(d) * kQSlots * 256u;
		QWideArgs w {};
		w.n_vectors   = nv;
		w.mask        = d_mask;
		w.zones       = d_zones;
		w.st          = state;
		w.bins        = pass_bins;
		w.cand        = cand;
		w.capacity    = cap;
		w.mask_hi     = mask_hi;
		w.shift       = shift;
		w.pass        = d;
		w.flush_every = tune.flush_every != 0 && tune.flush_every < kQFlushEvery ? tune.flush_every : kQFlushEvery;
		hipLaunchKernelGGL((k_quantile_wide<VB>), dim3(grid_wide), dim3(kQThreads), 0, stream, c, w);
		if (d > 0u) {
			QNarrowArgs n {};
			n.st       = state;
			n.cand     = cand;
			n.bins     = pass_bins;
			n.capacity = cap;
			n.mask_hi  = mask_hi;
			n.shift    = shift;
			n.pass     = d;
			hipLaunchKernelGGL(k_quantile_narrow, dim3(grid_narrow), dim3(kQThreads), 0, stream, n);
		}
		QPickArgs p {};
		p.capacity = cap;
		p.pass     = d;
		p.shift    = shift;
		p.vb       = VB;
		p.req      = req;
		hipLaunchKernelGGL(k_quantile_pick, dim3(1), dim3(1024), 0, stream, state, pass_bins, p);
		if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	}
	QFinishArgs f {};
	f.d_vals       = d_vals;
	f.d_ranks      = d_ranks;
	f.d_count      = d_count;
	f.n            = req.n;
	f.quantile     = req.quantile;
	f.wide_grid    = grid_wide;
	f.waves_per_wg = kQWaves;
	hipLaunchKernelGGL((k_quantile_finish<VB>), dim3(1), dim3(64), 0, stream, state, f);
	return hipGetLastError() == hipSuccess ? ALPGPU_OK : ALPGPU_ERR_HIP;
}

int launch_quantile(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, const void* d_zones, const double* q, const uint64_t* ranks, uint32_t n, int from_top,
                    void* d_vals, uint64_t* d_ranks, uint64_t* d_count, void* d_scratch, int value_bytes, int n_cus, const alpgpu_quantile_tuning* tuning) {
	QRequest req {};
	if (q != nullptr) {
		for (uint32_t i = 0; i < n; ++i) { req.q[i] = q[i]; }
		req.n        = 2u * n;
		req.quantile = 1u;
	} else {
		for (uint32_t i = 0; i < n; ++i) { req.ranks[i] = ranks[i]; }
		req.n        = n;
		req.from_top = from_top != 0;
	}
	const alpgpu_quantile_tuning tune = tuning != nullptr ? *tuning : alpgpu_quantile_tuning {};
	return value_bytes == 8 ? quantile<8>(stream, col, d_mask, d_zones, req, d_vals, d_ranks, d_count, d_scratch, n_cus, tune)
	                        : quantile<4>(stream, col, d_mask, d_zones, req, d_vals, d_ranks, d_count, d_scratch, n_cus, tune);
}

int quantile_trace(hipStream_t stream, const void* d_scratch, alpgpu_quantile_trace* out) {
	QState h;
	if (hipMemcpyAsync(&h, d_scratch, sizeof(QState), hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) { return ALPGPU_ERR_HIP; }
	out->compact_pass = h.compact_p1 != 0u ? h.compact_p1 - 1u : h.vb;
	out->wide_grid    = h.wide_grid;
	out->waves_per_wg = h.waves_per_wg;
	out->reserved     = 0;
	out->candidates   = h.n_cand;
	out->n            = h.n;
	out->zero_skips   = h.zero_skips;
	for (int i = 0; i < 8; ++i) { out->zone_skips[i] = h.zone_skips[i]; }
	return ALPGPU_OK;
}

} // namespace alpgpu
