// persistent_scan.hpp — the glue the persistent scan kernels share around the in-register decode of register_decode.hpp: k_in_list, k_join_probe,
// k_histogram, k_distinct_insert, k_quantile_wide, k_keyed_sum, k_keyed_minmax and k_keyed_minmax_many.  Each is workgroups that set their LDS up once, pass one barrier and then walk vectors
// v = wave id, wave id + waves, ... (k_keyed_sum: its wavefronts take stripes of consecutive vectors by a ticket and flush nothing: keyed_kernels.hip);
// what two or more of them do in the same way is stated here once: a vector's selected bits under a range and a nullable
// bitmap, the constant-vector shortcut's predicate and count, and the flush of 32-bit LDS bins into 64-bit global counts.  The sorted list in LDS
// and its search are sorted_list.hpp; the host's grid and staging rules are persistent_launch.hpp.
// The trip loop ("every wavefront of the workgroup makes the same number of trips, flush every flush_every") stays written out in k_histogram,
// k_distinct_insert and q_wide_loop: as one function template over the per-vector body and the flush, tried on k_histogram, it did not keep the
// kernel's instruction sequence (profiles/r24_persistent_scan.txt).
#pragma once
#include "register_decode.hpp"

namespace alpgpu {

// word m (= lane, < 16) of a vector's bitmap with the bits of the positions [p_begin, p_end) set
__device__ __forceinline__ uint64_t range_word(uint32_t lane, uint32_t p_begin, uint32_t p_end) {
	const uint32_t w0 = 64u * lane;
	const uint32_t lo = p_begin > w0 ? p_begin : w0, hi = p_end < w0 + 64u ? p_end : w0 + 64u;
	if (hi <= lo) { return 0ull; }
	const uint64_t run = hi - lo == 64u ? ~0ull : (1ull << (hi - lo)) - 1ull;
	return run << (lo - w0);
}

// The selected bits of vector v, lane m < 16 holding word m (the other lanes zero): the vector's 128 bytes of bitmap (all ones without one) ANDed
// with its share of the range [first, end) (the vector holds a value of the range: range_share).  false: no bit is set and nothing else of the
// vector need be read.
__device__ __forceinline__ bool selected_words(const uint64_t* mask, uint64_t first, uint64_t end, uint64_t v, uint32_t lane, uint64_t& sel) {
	uint32_t p_begin, p_end;
	range_share(first, end, v << 10, p_begin, p_end);
	sel = lane < 16u ? range_word(lane, p_begin, p_end) : 0ull;
	if (mask != nullptr) { sel &= lane < 16u ? mask[16ull * v + lane] : 0ull; }
	return ballot64(sel != 0ull) != 0ull;
}

// The constant-vector shortcut: a vector whose zone record pins all its numbers to one bucket or one value is settled from its selected bits alone
// if no selected value can be a NaN, and only a plain ALP vector without exceptions promises that: there a NaN is always an exception, while an
// ALP_RD vector can hold one in its packed words.  The count is then selected_count's.
__device__ __forceinline__ bool alp_without_exceptions(const alpgpu_vector_desc& d) { return d.scheme == ALPGPU_SCHEME_ALP && d.exc_cnt == 0u; }
// the set bits of selected_words' words, scanned over the lanes: lane 63 holds the vector's count
__device__ __forceinline__ uint32_t selected_count(uint64_t sel) { return wave_scan_add_u32(static_cast<uint32_t>(__builtin_popcountll(sel))); }

// The workgroup's (THREADS threads) non-zero 32-bit LDS bins into the 64-bit global counts by integer atomics; a barrier first, none behind.
template <int THREADS>
__device__ __forceinline__ void bins_flush(const uint32_t* s_bins, uint32_t n_bins, uint64_t* counts) {
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < n_bins; i += THREADS) {
		const uint32_t n = s_bins[i];
		if (n != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(counts) + i, static_cast<unsigned long long>(n)); }
	}
}
// the bins zeroed; no barrier.  (A flush in the middle of the trip loop is bins_flush, a barrier, bins_zero, a barrier, written out where it stands: as
// one function around the two it changed k_quantile_wide's register allocation.)
template <int THREADS>
__device__ __forceinline__ void bins_zero(uint32_t* s_bins, uint32_t n_bins) {
	for (uint32_t i = threadIdx.x; i < n_bins; i += THREADS) { s_bins[i] = 0u; }
}
} // namespace alpgpu
