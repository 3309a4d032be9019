// in_list_search.hpp — the search over a sorted list staged in LDS that k_in_list (in_list_kernels.hip) and k_join_probe (join_kernels.hip) share: the
// workgroup shape and the 32 KiB of list, the record that says what was staged (InArgs; k_join_probe leaves the bitmap fields zero) and in_list_search,
// the branch-free, wave-uniform bound with its pivot tier.  Only those two files include this header.
#pragma once
#include "launch.hpp"
#include "register_decode.hpp"

namespace alpgpu {

constexpr int      kInWaves    = 8; // wavefronts per workgroup: they share the staged list and nothing else
constexpr int      kInThreads  = 64 * kInWaves;
constexpr uint32_t kInLdsBytes = 32768; // of list per workgroup: 4096 doubles or 8192 floats; with the exception masks 33 KiB, four workgroups per CU
constexpr int      kInWgPerCu  = 4;

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

// NB searches side by side over the list's elements [j0, j1) (wave-uniform, j0 <= j1 <= n_list, n_list > 0): out[i] = j0 + the number of elements e
// of them with e < x[i] (bit i of `upper` set: e <= x[i]) if the list is sorted, in [j0, j1] whatever it holds.  A NaN element is never less, so
// that NaNs sorted last end the list; a NaN x gives j0.
template <int VB, bool GLOBAL, uint32_t NB>
__device__ __forceinline__ void in_list_search(const typename DecodeVec<VB>::T* s_list, const typename DecodeVec<VB>::T* list, const InArgs& g, uint32_t j0, uint32_t j1,
                                               const typename DecodeVec<VB>::T (&x)[NB], uint32_t upper, uint32_t (&out)[NB]) {
	typedef typename DecodeVec<VB>::T T;
	const uint32_t stride = GLOBAL ? g.stride : 1u;
	const uint32_t i0 = GLOBAL ? (j0 + stride - 1u) / stride : j0, i1 = GLOBAL ? (j1 + stride - 1u) / stride : j1; // the LDS words whose elements lie in [j0, j1)
	const uint32_t last_word = g.n_piv - 1u, last_elem = g.n_list - 1u;
	uint32_t       base[NB];
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
		n = stride - 1u;
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

} // namespace alpgpu
