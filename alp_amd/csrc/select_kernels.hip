// select_kernels.hip — range selection on a compressed column (alpgpu_select_range_*): which value indices r of [first, first + n) hold a value x
// with lo <= x <= hi, in ascending order, and optionally those values.  The decoded column never reaches HBM.
//
// Three phases, ordered by kernel boundaries on one stream (no workgroup ever waits for another):
//   count  k_select<VB, false>  one wavefront per vector decodes it in registers and writes counts[v] = its number of qualifying values (u32)
//          k_select<VB, false, const void*>  alpgpu_select_range_zoned_*: the same after a look at the vector's zone record {min, max}; a vector the record
//                               excludes, or admits whole, is counted from those 16 (8) bytes and its descriptor alone
//   scan   k_scan_*             exclusive prefix sum counts -> offsets (u64), blocks of 1024, block sums scanned the same way one level up;
//                               the top level writes *d_count
//   emit   k_select<VB, true>   one wavefront per vector: counts[v] == 0 -> gone after a 4-byte read; else the same decode again, and every
//                               qualifying value's index (and value) goes to offsets[v] + its rank inside the vector, if below the capacity
//
// The decode of one vector by one wavefront: 16 steps, step m holds value p = 64 m + lane in lane `lane`, so a wave-wide ballot of the predicate
// IS the 64 bits of the vector's qualify mask for indices 64 m .. 64 m + 63, in index order.  Rank inside the vector = qualifying values of the
// steps before (a wave-uniform running popcount) + the ballot's bits below the lane (v_mbcnt).  Ranks come from index-ordered masks and the
// offsets from a prefix sum, so the output ascends and is a function of the column and the arguments alone: no atomic decides a position.
// With p = 64 m + lane the lanes of a wavefront read neighbouring words of every stream (layouts: gather_kernels.hip):
//   ALP double   FastLanes lane p & 15 = lane & 15, row 4 m + (lane >> 4): four runs of 16 consecutive u64
//   ALP float    lane p & 31, row 2 m + (lane >> 5): two runs of 32 consecutive u32
//   ALP_RD left  lane p & 63 = lane, row m: 64 consecutive u16
// Exceptions: the record's ascending positions become a 1024-bit mask in the wavefront's 128 bytes of LDS (ds_or, as the store decode's
// ExcMask); step m reads its 64 bits, rank in the record = exceptions of the steps before + the mask's bits below the lane.  The packed words
// of eight steps are requested together, and in the source the exception values with them.  In the generated code that holds for ALP vectors
// only (three or four round trips to memory per vector instead of one per step); for ALP_RD vectors the compiler waits for each exception's
// left part right behind its load, so a step with an exception is a round trip of its own there (profiles/r08_select.txt).
// The arithmetic is the store decode's own (decode_value / decode_value_f32, the ALP_RD glue, the same tables, as gather_kernels.hip uses
// them), so a selected value has the bits alpgpu_decode_* writes at its index.
//
// HBM traffic: count reads every vector of the range once (descriptor, packed words, exception record, for ALP_RD the dictionary) and writes
// 4 bytes; the scan reads them and writes 8; emit reads 4 + 8 bytes per vector and, for vectors with a non-zero count only, the vector again,
// and writes 8 (+ 8 or 4) bytes per selected value.
#include <type_traits>

#include "alp_device_f32.hpp"
#include "lane_field.hpp"
#include "launch.hpp"

namespace alpgpu {

constexpr int      kSelWaves   = 4; // wavefronts per workgroup, one vector each (they share nothing)
constexpr int      kSelThreads = 64 * kSelWaves;
constexpr uint64_t kSelMaxGrid = 1ull << 30; // workgroups per launch
constexpr int      kScanBlock  = 1024;       // counts per scan block = threads per scan workgroup
constexpr uint32_t kSelBatch   = 8;          // steps of a vector whose words are requested together

// EMIT = false: counts[k] = qualifying values of vector v0 + k.  EMIT = true: their indices (and values) at offsets[k] + rank.
// [first, end) is the selected index range; the launch covers exactly the vectors it touches (v0 = first >> 10, n_range of them).
// ZONES: empty, or one `const void*` behind the other arguments = the zoned count pass of alpgpu_select_range_zoned_*: zones[v] = {min, max} (one
// record per vector of the COLUMN, indexed by v, not by v - v0) is read first.  A vector whose zone misses [lo, hi] is counted 0 and one whose
// zone lies inside it, and which cannot hold a NaN, is counted whole; neither has its packed words or exception record read.  (A trailing
// parameter pack and not a plain parameter: the unzoned instantiations keep their argument list and with it their instructions.)
__device__ __forceinline__ const void* zone_records(const void* zones) { return zones; }
template <int VB, bool EMIT, class... ZONES>
__global__ __launch_bounds__(kSelThreads) void k_select(const alpgpu_vector_desc* __restrict__ descs, const alpgpu_rowgroup_state* __restrict__ rgs,
                                                        const uint8_t* __restrict__ packed, const uint8_t* __restrict__ excs, uint64_t v0, uint64_t n_range,
                                                        uint64_t wg_off, uint64_t first, uint64_t end, double range_lo, double range_hi,
                                                        uint32_t* __restrict__ counts, const uint64_t* __restrict__ offsets, int64_t* __restrict__ d_idx,
                                                        void* __restrict__ d_vals, uint64_t capacity, ZONES... zones) {
	constexpr bool ZONED = sizeof...(ZONES) == 1;
	static_assert(sizeof...(ZONES) <= 1 && !(ZONED && EMIT), "at most the zone map, and the emit pass reads the counts, not the zones");
	typedef typename std::conditional<VB == 8, uint64_t, uint32_t>::type U;
	typedef typename std::conditional<VB == 8, double, float>::type      T;
	constexpr uint32_t kLanes = VB == 8 ? 16u : 32u; // FastLanes lanes of the value streams
	constexpr uint32_t kLog   = VB == 8 ? 4u : 5u;
	__shared__ uint64_t s_exc[kSelWaves][16]; // per wavefront: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t k    = (wg_off + blockIdx.x) * kSelWaves + wave;
	if (k >= n_range) { return; }
	const uint64_t v       = v0 + k;
	const uint64_t r0      = v << 10;
	const uint32_t p_begin = first > r0 ? static_cast<uint32_t>(first - r0) : 0u; // the vector's share of [first, end): wave-uniform
	const uint32_t p_end   = end - r0 < 1024u ? static_cast<uint32_t>(end - r0) : 1024u;

	uint32_t total = 0;
	uint64_t out0  = 0;
	if constexpr (EMIT) {
		total = counts[k];
		if (total == 0) { return; } // a vector without a qualifying value costs these four bytes
		out0 = offsets[k];
		if (out0 >= capacity) { return; }
		if (d_vals == nullptr && total == p_end - p_begin) { // all of it qualifies and only indices are wanted: nothing to decode
			for (uint32_t p = p_begin + lane; p < p_end; p += 64u) {
				const uint64_t j = out0 + (p - p_begin);
				if (j < capacity) { d_idx[j] = static_cast<int64_t>(r0 + p); }
			}
			return;
		}
	}

	bool inside = false; // ZONED: every value the zone admits qualifies
	if constexpr (ZONED) {
		const T* zone = reinterpret_cast<const T*>(zone_records(zones...)) + 2 * v; // (wave-uniform)
		const T  z_min = zone[0], z_max = zone[1];
		const T z_lo = static_cast<T>(range_lo), z_hi = static_cast<T>(range_hi);
		if (!(z_max >= z_lo && z_min <= z_hi)) { // excluded (a NaN bound excludes every vector): the record is all that was read
			if (lane == 0u) { counts[k] = 0u; }
			return;
		}
		inside = z_min >= z_lo && z_max <= z_hi;
	}
	const alpgpu_vector_desc d     = descs[v];
	const bool               alp   = d.scheme == ALPGPU_SCHEME_ALP;
	if constexpr (ZONED) {
		// contained: only a vector that cannot hold a NaN — ALP without exceptions (a NaN never round-trips through ALP, so it is always an exception)
		if (inside && alp && d.exc_cnt == 0u) {
			if (lane == 0u) { counts[k] = p_end - p_begin; }
			return;
		}
	}
	const uint32_t           bw    = d.bw < 8u * VB ? d.bw : 8u * VB;
	const uint32_t           cnt   = d.exc_cnt < 1024u ? d.exc_cnt : 1024u;
	const uint8_t*           rec   = excs + d.exc_off;
	const U*                 words = reinterpret_cast<const U*>(packed + d.packed_off);
	const uint16_t*          lefts = reinterpret_cast<const uint16_t*>(packed + d.packed_off + 128ull * d.bw);
	const U                  base  = static_cast<U>(d.base);
	// per-vector constants of the two schemes (gather_kernels.hip: value_bits reads the same tables with the same clamps)
	const uint32_t lbw  = d.lbw < 16u ? d.lbw : 16u;
	const uint32_t fi   = VB == 8 ? (d.f < 18 ? d.f : 18) : (d.f < 10 ? d.f : 10);
	const uint32_t ei   = VB == 8 ? (d.e < 20 ? d.e : 20) : (d.e < 10 ? d.e : 10);
	const RdDict   dict = load_rd_dict(rgs, v, !alp);
	const T        lo = static_cast<T>(range_lo), hi = static_cast<T>(range_hi);
	typename std::conditional<VB == 8, int64_t, uint32_t>::type fact;
	T                                                          frac;
	if constexpr (VB == 8) {
		fact = kFactArr[fi];
		frac = kFracArr[ei];
	} else {
		fact = kFactArrF[fi];
		frac = kFracArrF[ei];
	}

	if (cnt > 0) { // the exception positions as a mask in index order
		const uint16_t* pos = reinterpret_cast<const uint16_t*>(rec + (alp ? static_cast<uint64_t>(VB) : 2ull) * d.exc_cnt);
		if (lane < 16u) { s_exc[wave][lane] = 0ull; }
		wave_lds_sync();
		for (uint32_t j = lane; j < cnt; j += 64u) {
			const uint32_t q = pos[j];
			if (q < 1024u) { atomicOr(reinterpret_cast<uint32_t*>(&s_exc[wave][0]) + (q >> 5), 1u << (q & 31u)); }
		}
		wave_lds_sync();
	}

	uint32_t before_exc = 0; // exceptions of the steps done
	uint32_t before_sel = 0; // qualifying values of the steps done (wave-uniform: it comes from ballots)
	for (uint32_t b = 0; b < 16u; b += kSelBatch) {
		// every load of kSelBatch steps is requested before the first is used: a step is otherwise its own round trip to memory
		FieldWords<U>        rw[kSelBatch];
		FieldWords<uint16_t> lw[kSelBatch];
#pragma unroll
		for (uint32_t i = 0; i < kSelBatch; ++i) {
			rw[i] = FieldWords<U> {0, 0};
			lw[i] = FieldWords<uint16_t> {0, 0};
		}
		if (bw > 0) {
#pragma unroll
			for (uint32_t i = 0; i < kSelBatch; ++i) {
				const uint32_t p = 64u * (b + i) + lane;
				rw[i]            = load_field_words<U, kLanes>(words + (p & (kLanes - 1u)), p >> kLog, bw);
			}
		}
		if (!alp && lbw > 0) {
#pragma unroll
			for (uint32_t i = 0; i < kSelBatch; ++i) { lw[i] = load_field_words<uint16_t, 64>(lefts + lane, b + i, lbw); }
		}
		// ... the exceptions' values too (ALP: the value's bits; ALP_RD: its left part): loaded where they are used, each step with an exception in
		// it would wait for memory once more.  (The ALP_RD loads are still waited for one by one in the generated code, see the head of this file.
		// A form that avoids it was measured: every lane loads, without the per-lane branch, one loop per scheme.  It takes 98 registers
		// instead of 81 and cost the mixed and float columns more, +4 % and +8 %, than the ALP_RD column gained, -3 %.)
		uint64_t em[kSelBatch]; // wave-uniform: bit l = value 64 m + l is an exception
		U        ev[kSelBatch];
#pragma unroll
		for (uint32_t i = 0; i < kSelBatch; ++i) {
			em[i] = 0ull;
			ev[i] = 0;
		}
		if (cnt > 0) {
			uint32_t rank0 = before_exc;
#pragma unroll
			for (uint32_t i = 0; i < kSelBatch; ++i) {
				const uint64_t w = s_exc[wave][b + i];
				const uint32_t w_lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(w))); // (the builtin returns int: no sign extension into the high word)
				const uint32_t w_hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(w >> 32)));
				em[i]               = (static_cast<uint64_t>(w_hi) << 32) | w_lo;
				const uint32_t rank = rank0 + mbcnt64(em[i], 0u);
				if ((em[i] >> lane) & 1ull) { ev[i] = alp ? reinterpret_cast<const U*>(rec)[rank] : static_cast<U>(reinterpret_cast<const uint16_t*>(rec)[rank]); }
				rank0 += static_cast<uint32_t>(__builtin_popcountll(em[i]));
			}
			before_exc = rank0;
		}
#pragma unroll
		for (uint32_t i = 0; i < kSelBatch; ++i) {
			const uint32_t m     = b + i;
			const uint32_t p     = 64u * m + lane;
			const U        right = extract_field<U>(rw[i], p >> kLog, bw); // ALP: the digit; ALP_RD: the right part
			const bool     hit   = (em[i] >> lane) & 1ull;
			U              bits;
			if (alp) {
				if constexpr (VB == 8) {
					bits = static_cast<U>(__double_as_longlong(decode_value(static_cast<int64_t>(right + base), fact, frac)));
				} else {
					bits = __float_as_uint(decode_value_f32(static_cast<int32_t>(right + base), fact, frac));
				}
				bits = hit ? ev[i] : bits;
			} else {
				const uint32_t idx  = extract_field<uint16_t>(lw[i], m, lbw) & 7u;
				const U        left = hit ? ev[i] : static_cast<U>(((idx < 4u ? dict.lo : dict.hi) >> (16u * (idx & 3u))) & 0xFFFFull);
				bits                = static_cast<U>((left << bw) | right);
			}
			T x;
			if constexpr (VB == 8) { x = __longlong_as_double(static_cast<long long>(bits)); } else { x = __uint_as_float(bits); }
			const bool     q   = p >= p_begin && p < p_end && x >= lo && x <= hi; // NaN (value or bound) never qualifies; -0.0 == 0.0
			const uint64_t sel = ballot64(q);
			if constexpr (EMIT) {
				const uint64_t j = out0 + before_sel + mbcnt64(sel, 0u);
				if (q && j < capacity) {
					d_idx[j] = static_cast<int64_t>(r0 + p);
					if (d_vals != nullptr) { reinterpret_cast<U*>(d_vals)[j] = bits; }
				}
			}
			before_sel += static_cast<uint32_t>(__builtin_popcountll(sel));
		}
		if constexpr (EMIT) {
			if (before_sel >= total || out0 + before_sel >= capacity) { return; } // the vector's last qualifying value, or the capacity, is behind us
		}
	}
	if constexpr (!EMIT) {
		if (lane == 0u) { counts[k] = before_sel; }
	}
}

// ---- the scan: out[i] = in[0] + ... + in[i - 1] --------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
	for (int s = 32; s > 0; s >>= 1) { x += __shfl_xor(x, s, 64); }
	return x;
}

// sums[b] = in[1024 b] + ... + in[1024 b + 1023]
template <class T>
__global__ __launch_bounds__(kScanBlock) void k_scan_reduce(const T* __restrict__ in, uint64_t n, uint64_t* __restrict__ sums) {
	__shared__ uint64_t s_wave[kScanBlock / 64];
	const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
	const uint64_t x = wave_sum(i < n ? static_cast<uint64_t>(in[i]) : 0ull);
	if ((threadIdx.x & 63u) == 0u) { s_wave[threadIdx.x >> 6] = x; }
	__syncthreads();
	if (threadIdx.x == 0) {
		uint64_t t = 0;
		for (int w = 0; w < kScanBlock / 64; ++w) { t += s_wave[w]; }
		sums[blockIdx.x] = t;
	}
}

// out[i] = block_off[b] + the sum of the block's elements before i (block_off == nullptr: one block, offset 0).  total (nullable): the sum of
// everything, written by the launch's last block — the caller passes it on the top level only.  in == out is allowed when T is uint64_t.
template <class T>
__global__ __launch_bounds__(kScanBlock) void k_scan_apply(const T* in, uint64_t n, const uint64_t* __restrict__ block_off, uint64_t* out, uint64_t* __restrict__ total) {
	__shared__ uint64_t s_wave[kScanBlock / 64];
	const uint64_t i    = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint64_t x    = i < n ? static_cast<uint64_t>(in[i]) : 0ull;
	uint64_t       incl = x;
	for (int s = 1; s < 64; s <<= 1) {
		const uint64_t y = __shfl_up(incl, s, 64);
		if (lane >= static_cast<uint32_t>(s)) { incl += y; }
	}
	if (lane == 63u) { s_wave[wave] = incl; }
	__syncthreads();
	uint64_t before = block_off ? block_off[blockIdx.x] : 0ull;
	for (uint32_t w = 0; w < wave; ++w) { before += s_wave[w]; }
	if (i < n) { out[i] = before + incl - x; }
	if (total != nullptr && blockIdx.x == gridDim.x - 1 && threadIdx.x == kScanBlock - 1) { *total = before + incl; }
}

static uint64_t align16(uint64_t x) { return (x + 15ull) & ~15ull; }
static uint64_t scan_blocks(uint64_t n) { return (n + kScanBlock - 1) / kScanBlock; }

// Scratch of a select over a column of n_vectors: [offsets: u64 per vector][counts: u32 per vector][block sums of every scan level], each
// part rounded up to 16 bytes.  The levels shrink by 1024 each (n_vectors / 1024 + 1, that / 1024 + 1, ... down to one block: at most six
// for any n_vectors below 2^54), so the whole is at most 12 * n_vectors + n_vectors / 100 + 256 bytes.
uint64_t select_scratch_bytes(uint64_t n_vectors) {
	if (n_vectors > (1ull << 54)) { return ~0ull; }
	uint64_t bytes = align16(8ull * n_vectors) + align16(4ull * n_vectors);
	for (uint64_t len = n_vectors; len > kScanBlock;) {
		len = scan_blocks(len);
		bytes += align16(8ull * len);
	}
	return bytes < 16ull ? 16ull : bytes;
}

template <class T>
static int scan_level(hipStream_t stream, const T* in, uint64_t n, uint64_t* out, uint64_t* d_total, uint64_t* levels) {
	const uint64_t nb = scan_blocks(n);
	if (nb > 0x7FFFFFFFull) { return ALPGPU_ERR_INVALID; }
	if (nb <= 1) {
		hipLaunchKernelGGL((k_scan_apply<T>), dim3(1), dim3(kScanBlock), 0, stream, in, n, static_cast<const uint64_t*>(nullptr), out, d_total);
		return hipGetLastError() == hipSuccess ? ALPGPU_OK : ALPGPU_ERR_HIP;
	}
	hipLaunchKernelGGL((k_scan_reduce<T>), dim3(static_cast<unsigned>(nb)), dim3(kScanBlock), 0, stream, in, n, levels);
	if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	const int rc = scan_level<uint64_t>(stream, levels, nb, levels, d_total, levels + align16(8ull * nb) / 8ull); // the block sums, scanned in place one level up
	if (rc != ALPGPU_OK) { return rc; }
	hipLaunchKernelGGL((k_scan_apply<T>), dim3(static_cast<unsigned>(nb)), dim3(kScanBlock), 0, stream, in, n, static_cast<const uint64_t*>(levels), out,
	                   static_cast<uint64_t*>(nullptr));
	return hipGetLastError() == hipSuccess ? ALPGPU_OK : ALPGPU_ERR_HIP;
}

// d_offsets[i] = d_counts[0] + ... + d_counts[i - 1], *d_total = the sum of all n (n > 0); d_levels: the block-sum part of the scratch
int launch_select_scan(hipStream_t stream, const uint32_t* d_counts, uint64_t n, uint64_t* d_offsets, uint64_t* d_total, uint64_t* d_levels) {
	return scan_level<uint32_t>(stream, d_counts, n, d_offsets, d_total, d_levels);
}

template <int VB, bool EMIT>
static int launch_select_pass(hipStream_t stream, const alpgpu_column* col, uint64_t v0, uint64_t n_range, uint64_t first, uint64_t end, double lo, double hi,
                              uint32_t* counts, const uint64_t* offsets, int64_t* d_idx, void* d_vals, uint64_t capacity) {
	const uint64_t n_wg = (n_range + kSelWaves - 1) / kSelWaves;
	for (uint64_t off = 0; off < n_wg; off += kSelMaxGrid) {
		const uint64_t g = n_wg - off < kSelMaxGrid ? n_wg - off : kSelMaxGrid;
		hipLaunchKernelGGL((k_select<VB, EMIT>), dim3(static_cast<unsigned>(g)), dim3(kSelThreads), 0, stream, col->d_vectors, col->d_rowgroups, col->d_packed, col->d_exc,
		                   v0, n_range, off, first, end, lo, hi, counts, offsets, d_idx, d_vals, capacity);
		if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	}
	return ALPGPU_OK;
}

template <int VB>
static int launch_select_count_zoned(hipStream_t stream, const alpgpu_column* col, const void* d_zones, uint64_t v0, uint64_t n_range, uint64_t first, uint64_t end,
                                     double lo, double hi, uint32_t* counts) {
	const uint64_t n_wg = (n_range + kSelWaves - 1) / kSelWaves;
	for (uint64_t off = 0; off < n_wg; off += kSelMaxGrid) {
		const uint64_t g = n_wg - off < kSelMaxGrid ? n_wg - off : kSelMaxGrid;
		hipLaunchKernelGGL((k_select<VB, false, const void*>), dim3(static_cast<unsigned>(g)), dim3(kSelThreads), 0, stream, col->d_vectors, col->d_rowgroups, col->d_packed,
		                   col->d_exc, v0, n_range, off, first, end, lo, hi, counts, static_cast<const uint64_t*>(nullptr), static_cast<int64_t*>(nullptr), static_cast<void*>(nullptr),
		                   0ull, d_zones);
		if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	}
	return ALPGPU_OK;
}

// n > 0 and first + n <= n_vectors * 1024 (the caller checked); d_scratch: select_scratch_bytes(col->n_vectors) bytes, 16-byte aligned
// d_zones (nullable): the column's zone map, one record per vector — the count pass then reads a vector's record before the vector
int launch_select_range(hipStream_t stream, const alpgpu_column* col, uint64_t first, uint64_t n, double lo, double hi, int64_t* d_idx, void* d_vals,
                        uint64_t capacity, uint64_t* d_count, void* d_scratch, int value_bytes, const void* d_zones) {
	const uint64_t end     = first + n;
	const uint64_t v0      = first >> 10;
	const uint64_t n_range = ((end - 1) >> 10) - v0 + 1;
	uint64_t*      offsets = static_cast<uint64_t*>(d_scratch);
	uint32_t*      counts  = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(d_scratch) + align16(8ull * col->n_vectors));
	uint64_t*      levels  = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(counts) + align16(4ull * col->n_vectors));
	int            rc;
	if (d_zones != nullptr) {
		rc = value_bytes == 8 ? launch_select_count_zoned<8>(stream, col, d_zones, v0, n_range, first, end, lo, hi, counts)
		                      : launch_select_count_zoned<4>(stream, col, d_zones, v0, n_range, first, end, lo, hi, counts);
	} else {
		rc = value_bytes == 8 ? launch_select_pass<8, false>(stream, col, v0, n_range, first, end, lo, hi, counts, nullptr, nullptr, nullptr, 0)
		                      : launch_select_pass<4, false>(stream, col, v0, n_range, first, end, lo, hi, counts, nullptr, nullptr, nullptr, 0);
	}
	if (rc != ALPGPU_OK) { return rc; }
	rc = launch_select_scan(stream, counts, n_range, offsets, d_count, levels);
	if (rc != ALPGPU_OK || capacity == 0) { return rc; }
	return value_bytes == 8 ? launch_select_pass<8, true>(stream, col, v0, n_range, first, end, lo, hi, counts, offsets, d_idx, d_vals, capacity)
	                        : launch_select_pass<4, true>(stream, col, v0, n_range, first, end, lo, hi, counts, offsets, d_idx, d_vals, capacity);
}

} // namespace alpgpu
