// sorted_list.hpp — a sorted list staged in LDS and searched there, the one home of it: lds_bound, the branch-free, wave-uniform bound over LDS
// words that k_in_list (in_list_kernels.hip), k_join_probe (join_kernels.hip), k_histogram (histogram_kernels.hip: its edges), k_keyed_sum
// (keyed_kernels.hip: its keys), k_keyed_minmax (keyed_minmax_kernels.hip: its keys) and k_bucket_sum / k_bucket_minmax (bucket_kernels.hip: their edges) share, and, for the first two and k_keyed_minmax_many
// (keyed_minmax_many_kernels.hip) and k_keyed_sum_exact (keyed_sum_exact_kernels.hip), the workgroup shape, the record that says what was staged (InArgs; k_join_probe, k_keyed_minmax_many and k_keyed_sum_exact leave
// the bitmap fields zero), the staging loop, in_list_search with its pivot tier, the zone bounds and the fetch for the equality test.  Only those
// eight files include this header, the last five through keyed_table.hpp.
#pragma once
#include "launch.hpp"
#include "register_decode.hpp"

namespace alpgpu {

constexpr int kInWaves   = 8; // wavefronts per workgroup: they share the staged list and nothing else
constexpr int kInThreads = 64 * kInWaves;
constexpr int kInWgPerCu = 4; // kInLdsBytes of list (persistent_launch.hpp) and the exception masks: 33 KiB each

struct InArgs {
	uint64_t    v0, n_range; // the launch covers vectors v0 + [0, n_range)
	uint64_t    first, end;  // the selected index range
	uint64_t*   mask;        // combined and stored
	const void* list;        // n_list sorted elements of the column's type
	const void* zones;       // nullable: one record {min, max} per vector of the COLUMN
	uint32_t    n_list;      // <= 2^31 - 1
	uint32_t    stride;      // LDS word i = list[i * stride]; 1 unless GLOBAL
	uint32_t    n_piv;       // LDS words staged: ceil(n_list / stride) <= kInLdsBytes / VB
	int         op;          // kMaskSet / kMaskAnd / kMaskOr
	int         negate;
};

// NB searches side by side over the LDS words [i0, i1) (wave-uniform, i0 <= i1): out[i] = i0 + the number of words e of them with e < x[i] (bit i
// of `upper` set: e <= x[i]) if the words are sorted, in [i0, i1] whatever they hold.  A NaN word is never less, so that NaNs sorted last end the
// list; a NaN x gives i0.  Every probe index is clamped to last_word, the last word staged (0 when none is); with i0 == i1 no word is read.
template <class T, uint32_t NB>
__device__ __forceinline__ void lds_bound(const T* s_list, uint32_t last_word, uint32_t i0, uint32_t i1, const T (&x)[NB], uint32_t upper, uint32_t (&out)[NB]) {
	uint32_t base[NB]; // (an array of its own, copied out at the end: grown in the caller's, k_in_list's instructions change)
#pragma unroll
	for (uint32_t i = 0; i < NB; ++i) { base[i] = i0; }
	uint32_t n = i1 - i0; // wave-uniform: every lane and every one of the NB searches takes the same steps
	while (n > 1u) {
		const uint32_t half = n >> 1;
		T              e[NB];
#pragma unroll
		for (uint32_t i = 0; i < NB; ++i) {
			const uint32_t at = base[i] + half - 1u;
			e[i]              = s_list[at < last_word ? at : last_word];
		}
#pragma unroll
		for (uint32_t i = 0; i < NB; ++i) { base[i] += (((upper >> i) & 1u) ? e[i] <= x[i] : e[i] < x[i]) ? half : 0u; }
		n -= half;
	}
	if (n == 1u) {
		T e[NB];
#pragma unroll
		for (uint32_t i = 0; i < NB; ++i) { e[i] = s_list[base[i] < last_word ? base[i] : last_word]; }
#pragma unroll
		for (uint32_t i = 0; i < NB; ++i) { base[i] += (((upper >> i) & 1u) ? e[i] <= x[i] : e[i] < x[i]) ? 1u : 0u; }
	}
#pragma unroll
	for (uint32_t i = 0; i < NB; ++i) { out[i] = base[i]; }
}

// The list (GLOBAL: its pivots) into LDS, by the whole workgroup, once; the caller's one workgroup barrier follows.
template <int VB, bool GLOBAL>
__device__ __forceinline__ void sorted_list_stage(typename DecodeVec<VB>::T* s_list, const typename DecodeVec<VB>::T* list, const InArgs& g) {
	for (uint32_t i = threadIdx.x; i < g.n_piv; i += kInThreads) {
		const uint64_t at = static_cast<uint64_t>(i) * (GLOBAL ? g.stride : 1u);
		s_list[i]         = list[at < g.n_list ? at : g.n_list - 1u]; // (n_piv > 0 only with n_list > 0)
	}
}

// NB searches side by side over the list's elements [j0, j1) (wave-uniform, j0 <= j1 <= n_list, n_list > 0): out[i] = j0 + the number of elements e
// of them with e < x[i] (bit i of `upper` set: e <= x[i]) if the list is sorted, in [j0, j1] whatever it holds: lds_bound over the words whose
// elements lie in [j0, j1) and, GLOBAL, the same steps over the list's slice between two pivots.
template <int VB, bool GLOBAL, uint32_t NB>
__device__ __forceinline__ void in_list_search(const typename DecodeVec<VB>::T* s_list, const typename DecodeVec<VB>::T* list, const InArgs& g, uint32_t j0, uint32_t j1,
                                               const typename DecodeVec<VB>::T (&x)[NB], uint32_t upper, uint32_t (&out)[NB]) {
	typedef typename DecodeVec<VB>::T T;
	const uint32_t stride = GLOBAL ? g.stride : 1u;
	const uint32_t i0 = GLOBAL ? (j0 + stride - 1u) / stride : j0, i1 = GLOBAL ? (j1 + stride - 1u) / stride : j1; // the LDS words whose elements lie in [j0, j1)
	const uint32_t last_word = g.n_piv - 1u, last_elem = g.n_list - 1u;
	uint32_t       base[NB];
	lds_bound<T, NB>(s_list, last_word, i0, i1, x, upper, base);
	if constexpr (!GLOBAL) {
#pragma unroll
		for (uint32_t i = 0; i < NB; ++i) { out[i] = base[i]; }
	} else {
		// base = p in [i0, i1]: word p - 1 is less (or p == i0) and word p is not (or p == i1), so the bound lies in the list's slice
		// [lo, hi], hi - lo <= stride - 1.  The same steps over a window of stride - 1 elements from lo on, those at or behind hi never less.
		uint32_t lo[NB], hi[NB];
#pragma unroll
		for (uint32_t i = 0; i < NB; ++i) {
			const uint32_t p = base[i];
			lo[i]            = p == i0 ? j0 : (p - 1u) * stride + 1u;
			hi[i]            = p * stride < j1 ? p * stride : j1;
		}
		uint32_t n = stride - 1u;
		while (n > 1u) {
			const uint32_t half = n >> 1;
			T              e[NB];
#pragma unroll
			for (uint32_t i = 0; i < NB; ++i) {
				const uint32_t at = lo[i] + half - 1u;
				e[i]              = list[at < last_elem ? at : last_elem];
			}
#pragma unroll
			for (uint32_t i = 0; i < NB; ++i) {
				const uint32_t at = lo[i] + half - 1u;
				lo[i] += (at < hi[i] && (((upper >> i) & 1u) ? e[i] <= x[i] : e[i] < x[i])) ? half : 0u;
			}
			n -= half;
		}
		if (n == 1u) {
			T e[NB];
#pragma unroll
			for (uint32_t i = 0; i < NB; ++i) { e[i] = list[lo[i] < last_elem ? lo[i] : last_elem]; }
#pragma unroll
			for (uint32_t i = 0; i < NB; ++i) { lo[i] += (lo[i] < hi[i] && (((upper >> i) & 1u) ? e[i] <= x[i] : e[i] < x[i])) ? 1u : 0u; }
		}
#pragma unroll
		for (uint32_t i = 0; i < NB; ++i) { out[i] = lo[i]; }
	}
}

// The part [j0, j1) of the list that vector v's zone record {min, max} admits, wave-uniform: j0 = the first element >= min, j1 = the first element
// > max, searched by the whole wavefront (every lane the same probes); a NaN bound leaves j0, j1 as they are.  j1 <= j0: no element lies in the record.
// g.zones non-null and n_list > 0: the kernels begin with j0 = 0, j1 = n_list and test the two in front of the call (tested in here, their instructions change).
template <int VB, bool GLOBAL>
__device__ __forceinline__ void sorted_list_zone(const typename DecodeVec<VB>::T* s_list, const typename DecodeVec<VB>::T* list, const InArgs& g, uint64_t v, uint32_t& j0,
                                                 uint32_t& j1) {
	typedef typename DecodeVec<VB>::T T;
	const T* zone = static_cast<const T*>(g.zones) + 2 * v; // (wave-uniform)
	const T  z[2] = {zone[0], zone[1]};
	if (z[0] == z[0] && z[1] == z[1]) {
		uint32_t j[2];
		in_list_search<VB, GLOBAL, 2>(s_list, list, g, 0u, g.n_list, z, 2u, j);
		j0 = __builtin_amdgcn_readfirstlane(j[0]);
		j1 = __builtin_amdgcn_readfirstlane(j[1]);
	}
}

// the element at a bound `at` of in_list_search (<= n_list), clamped to the list: what the one == behind the search compares with
template <int VB, bool GLOBAL>
__device__ __forceinline__ typename DecodeVec<VB>::T sorted_list_at(const typename DecodeVec<VB>::T* s_list, const typename DecodeVec<VB>::T* list, const InArgs& g, uint32_t at) {
	if constexpr (GLOBAL) { return list[at < g.n_list - 1u ? at : g.n_list - 1u]; } else { return s_list[at < g.n_piv - 1u ? at : g.n_piv - 1u]; }
}

} // namespace alpgpu
