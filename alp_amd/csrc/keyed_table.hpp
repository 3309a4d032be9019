// keyed_table.hpp — what the aggregations over a value column decoded beside a key column share: keyed SUM (keyed_kernels.hip), keyed MIN / MAX
// (keyed_minmax_kernels.hip), keyed MIN / MAX for many keys (keyed_minmax_many_kernels.hip), bucketed SUM and MIN / MAX (bucket_kernels.hip) and the
// exact keyed SUM (keyed_sum_exact_kernels.hip: of this header's own pieces it uses the trace's classes alone, and through it the headers included
// below).  Only those five files include this header.  It holds the LEAF pieces of the two kinds of table (the sum table: a private table per wavefront fed by
// keyed_step; the record table: one table per workgroup fed by kmm_step), the trace's classes, the tiers and the declarations of the two kernels that
// bucket_kernels.hip launches from keyed_kernels.hip.
//
// Why no more than that.  With these pieces here all 18 kernels of the four files compile to the device assembly they compiled to with their own
// copies (profiles/r29_keyed_tables.txt, part 1).  Every larger piece that was tried behind a __forceinline__ call (the one-entry paths, the trace's
// epilogue, the vector functions and kernel bodies as templates over a search policy) changes the compiler's register assignment and schedule in
// some kernel, and some of those kernels then ran 1 - 3 % behind; the vector functions and kernel bodies therefore stay in their files (DESIGN.md,
// "Keyed aggregation": which kernel, by what; the profile's part 2 has the shapes).  A piece moves here once it is shown to leave the assembly as it is.
#pragma once
#include "minmax_device.hpp"
#include "persistent_scan.hpp"
#include "sorted_list.hpp"

namespace alpgpu {

// keyed_kernels.hip's, launched by bucket_kernels.hip too: the counts and the scratch's header zeroed; out[key] = k_tree_sum's tree over the key's
// column of the partials
__global__ void k_keyed_init(uint64_t* counts, uint32_t n_counts, uint64_t* header);
__global__ void k_keyed_reduce(const double* __restrict__ partials, uint32_t n_stripes, uint32_t n_keys, double* __restrict__ out);

// The sum table's two capacity tiers, in table entries (keys, or buckets = edges + 1: bucket_kernels.hip uses the keyed kernels' values on purpose), so that a call with few entries is not held to the occupancy of 1024: 256 with 8 wavefronts
// (two workgroups per CU, what the registers admit under 4 waves per SIMD), ALPGPU_KEYED_KEYS_MAX = 1024 with 12 wavefronts (one workgroup per CU,
// what the LDS admits).
constexpr uint32_t kKeyedSmallKeys = 256u;
constexpr int      kKeyedSmallWaves = 8, kKeyedLargeWaves = 12;
constexpr int      kKeyedSmallWgPerCu = 2, kKeyedLargeWgPerCu = 1;
// The record table's one tier, 1 .. ALPGPU_KEYED_KEYS_MAX entries (keyed_minmax_kernels.hip says why 8 wavefronts and two workgroups per CU); bucketed too.
constexpr int      kKmmWaves      = 8;
constexpr int      kKmmThreads    = 64 * kKmmWaves;
constexpr int      kKmmWgPerCu    = 2;
constexpr uint32_t kKmmFlushEvery = 1u << 18; // trips of a workgroup's loop (8 vectors each, at most 8192 increments of one 32-bit LDS count) between two count flushes

// ---- the trace ---------------------------------------------------------------------------------------------------------------------------------------

// what a vector function (keyed_vector, kmm_vector, kmany_vector, bucket_sum_vector, bucket_mm_vector) did with a vector: the trace's words (include/alpgpu.h)
constexpr uint32_t kVectorSkipZero = 0u; // no selected row: neither column read
constexpr uint32_t kVectorOneEntry = 1u; // the zone record names one entry and the key vector is ALP without exceptions: the value vector alone decoded
constexpr uint32_t kVectorNoEntry  = 2u; // the zone record admits no key: neither column read (never returned by the bucketed kernels)
constexpr uint32_t kVectorDecoded  = 3u; // both vectors decoded

// ---- the sum table: a PRIVATE table per wavefront of doubles and 32-bit counts in LDS ------------------------------------------------------------------

// One step's member lanes m (wave-uniform) into the wavefront's table: lane l holds the value x and the entry idx (in the table where its bit of m is set).
__device__ __forceinline__ void keyed_step(double* s_sums, uint32_t* s_cnt, uint64_t m, uint32_t idx, double x, uint32_t lane) {
	if (m == 0ull) { return; }
	const bool     in    = (m >> lane) & 1ull;
	const uint32_t first = static_cast<uint32_t>(__builtin_amdgcn_readlane(idx, static_cast<uint32_t>(__builtin_ctzll(m))));
	uint64_t       same  = m & ballot64(idx == first);
	if (same == m) { // the step's lanes agree on one entry
		const double p = wave_tree_sum_f64(in ? x : 0.0);
		if (lane == 0u) {
			s_sums[first] += p;
			s_cnt[first] += static_cast<uint32_t>(__builtin_popcountll(m));
		}
		wave_lds_sync(); // (as every exit of this function: the next step's first LDS access, of any lane, comes behind lane 0's)
		return;
	}
	// the counts of all of m by one LDS atomic; a lane that saw its entry's count grow by exactly 1 is alone with that entry in this step
	const uint32_t c0 = in ? s_cnt[idx] : 0u;
	wave_lds_sync();
	if (in) { atomicAdd(&s_cnt[idx], 1u); }
	wave_lds_sync();
#ifndef ALPGPU_KEYED_BASELINE_STEP
	const uint32_t c1    = in ? s_cnt[idx] : 0u;
	const uint64_t alone = ballot64(in && c1 - c0 == 1u);
	if ((alone >> lane) & 1ull) { s_sums[idx] += x; } // 64 different addresses
	wave_lds_sync();
	uint64_t left = m & ~alone;
#else // the measurement's baseline (tools/time_keyed.py --ab): every entry of the step through ballot, tree and lane 0; the same bits
	(void)c0;
	uint64_t left = m;
#endif
	while (left != 0ull) { // entry by entry, in the order of the entries' first lanes
		const uint32_t i = static_cast<uint32_t>(__builtin_amdgcn_readlane(idx, static_cast<uint32_t>(__builtin_ctzll(left))));
		same             = left & ballot64(idx == i);
		const double p   = wave_tree_sum_f64(((same >> lane) & 1ull) ? x : 0.0);
		if (lane == 0u) { s_sums[i] += p; }
		left &= ~same;
	}
	wave_lds_sync();
}

// ---- the record table: ONE table per workgroup of {mn, mx, cnt} in LDS on integer atomics -------------------------------------------------------------

// the records' order as a signed integer: the value's bits, the negative half turned round (-0.0 -> -1, just below +0.0 -> 0); x is not a NaN
__device__ __forceinline__ long long order_key(double x) {
	const long long b = __double_as_longlong(x);
	return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFFll);
}
__device__ __forceinline__ int order_key(float x) {
	const int b = static_cast<int>(__float_as_uint(x));
	return b ^ ((b >> 31) & 0x7FFFFFFF);
}

// a wave-uniform record {mn, mx} (lane 0 acts) into entry i of the table, unless it is the empty one
template <class T>
__device__ __forceinline__ void kmm_join(T* s_mn, T* s_mx, uint32_t i, T mn, T mx, uint32_t lane) {
	if (lane == 0u && mn <= mx) { // ({+inf, -inf}: no number was fed; -0.0 <= +0.0 and inf <= inf hold)
		atomic_min_value(&s_mn[i], mn);
		atomic_max_value(&s_mx[i], mx);
	}
}

// One step's member lanes m (wave-uniform) into the workgroup's table: lane l holds the canonical value q and the entry idx (in the table where its bit of m is set).
template <class T>
__device__ __forceinline__ void kmm_step(T* s_mn, T* s_mx, uint32_t* s_cnt, bool counted, uint64_t m, uint32_t idx, T q, uint32_t lane) {
	if (m == 0ull) { return; }
	const bool     in    = (m >> lane) & 1ull;
	const uint32_t first = static_cast<uint32_t>(__builtin_amdgcn_readlane(idx, static_cast<uint32_t>(__builtin_ctzll(m))));
	if ((m & ballot64(idx == first)) == m) { // the step's lanes agree on one entry
		T mn = pos_inf<T>(), mx = -pos_inf<T>();
		minmax_feed(mn, mx, in ? q : minmax_skip<T>()); // (a NaN q is a quiet one: skipped)
		wave_minmax<T>(mn, mx);
		kmm_join(s_mn, s_mx, first, mn, mx, lane);
		if (counted && lane == 0u) { atomicAdd(&s_cnt[first], static_cast<uint32_t>(__builtin_popcountll(m))); }
		return;
	}
	if (in) {
		if (q == q) {
#ifndef ALPGPU_KEYED_MINMAX_NO_GUARD
			// an atomic only where the value improves on what a plain load read, compared by the records' INTEGER order key (C's < would drop a -0.0
			// that arrives behind +0.0).  A stale read is safe: the table moves one way, so it can cause a needless atomic and never a missed one.
			const auto k = order_key(q);
			if (k < order_key(s_mn[idx])) { atomic_min_value(&s_mn[idx], q); }
			if (k > order_key(s_mx[idx])) { atomic_max_value(&s_mx[idx], q); }
#else // the measurement's other arm (tools/time_keyed_minmax.py --ab): every number issues both atomics; the same bits
			atomic_min_value(&s_mn[idx], q);
			atomic_max_value(&s_mx[idx], q);
#endif
		}
		if (counted) { atomicAdd(&s_cnt[idx], 1u); }
	}
}

// the workgroup's non-zero LDS counts into the call's and zeroed again; a barrier in front and behind
__device__ __forceinline__ void kmm_counts_flush(uint32_t* s_cnt, uint32_t n, uint64_t* counts) {
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < n; i += kKmmThreads) {
		const uint32_t c = s_cnt[i];
		if (c != 0u) {
			atomicAdd(reinterpret_cast<unsigned long long*>(counts) + i, static_cast<unsigned long long>(c));
			s_cnt[i] = 0u;
		}
	}
	__syncthreads();
}

} // namespace alpgpu
