// in_list_kernels.hip — set membership (include/alpgpu.h, "set membership": alpgpu_select_in_mask_*): `x IN (list)` on a compressed column into a
// selection bitmap.
//
//   k_in_list<VB, GLOBAL>   persistent workgroups of kInWaves wavefronts.  The workgroup stages the sorted list (or, GLOBAL, every stride-th element
//                           of it: the pivots) into 32 KiB of static LDS, passes ONE workgroup barrier and only then walks vectors
//                           v = wave_id, wave_id + n_waves, ...: every early-out of the skip rules sits behind that barrier.  A vector is decoded in
//                           registers by register_decode.hpp in batches of kStepBatch steps, whose values search together, so that their LDS
//                           (and global) probes overlap.  The ballot of step m is kept in lane m, combined with the prior words and stored as
//                           one run of 128 bytes, as the MASK arm of k_select does.
//   the search              (in_list_search, sorted_list.hpp: shared with k_join_probe, its LDS tier with k_histogram too) a branch-free lower bound, every step wave-uniform in its length: ceil(log2(n + 1)) probes of the LDS words
//                           [i0, i1), then, GLOBAL, ceil(log2(stride)) probes of the list itself on the slice between two pivots (stride - 1
//                           elements at most; elements behind the slice's end count as "not less"), then one ==.  Every probe index is clamped to
//                           the words staged and to the list: an unsorted list gives unspecified bits and reads nothing else.
//   zones                   a vector's record {min, max} is searched twice by the whole wavefront (the same routine, every lane the same probes):
//                           j0 = the first element >= min, j1 = the first element > max.  j1 <= j0: no element lies in the record and the vector is
//                           settled from its 128 bytes of bitmap; else the per-value search runs over [j0, j1) only.
//
// HBM traffic per vector: the bitmap's 128 bytes and, unless they (or the zone record) settle the vector, its descriptor, packed words and exception
// record; the list once per workgroup.  One launch of at most 4 workgroups per CU (what 33 KiB of LDS each allow), whatever the column's length.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; launch bounds 512 = 2 wavefronts per SIMD and workgroup):
//   k_in_list<8, false>   83 VGPRs, 33792 B LDS, 5 waves per SIMD, no scratch
//   k_in_list<8, true>    79 VGPRs, 33792 B LDS, 6 waves per SIMD, no scratch
//   k_in_list<4, false>   75 VGPRs, 33792 B LDS, 6 waves per SIMD, no scratch
//   k_in_list<4, true>    71 VGPRs, 33792 B LDS, 7 waves per SIMD, no scratch
#include "persistent_scan.hpp"
#include "sorted_list.hpp"

namespace alpgpu {

template <int VB, bool GLOBAL>
__global__ __launch_bounds__(kInThreads) void k_in_list(const ColumnStreams c, const InArgs g) {
	typedef typename DecodeVec<VB>::T T;
	__shared__ T        s_list[kInLdsBytes / VB];
	__shared__ uint64_t s_exc[kInWaves][16]; // per wavefront: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const T*       list = static_cast<const T*>(g.list);

	// 0. the list (GLOBAL: its pivots) into LDS, once per workgroup; the one workgroup barrier of the kernel
	sorted_list_stage<VB, GLOBAL>(s_list, list, g);
	__syncthreads();

	const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * kInWaves;
	for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * kInWaves + wave; k < g.n_range; k += n_waves) {
		const uint64_t v  = g.v0 + k;
		const uint64_t r0 = v << 10;
		uint64_t*      mw = g.mask + 16ull * v;

		// 1. the vector's 128 bytes of bitmap, lane m < 16 holding word m, and what they settle without the column
		// (the rules of k_select's MASK arm; written out in each of the three kernels that write a bitmap: the note at the end of register_decode.hpp)
		uint64_t   prior   = 0;
		const bool outside = r0 >= g.end || r0 + 1024u <= g.first; // no value of the vector is in the range: q is false throughout
		if (g.op == kMaskSet) {
			if (outside) {
				if (lane < 16u) { mw[lane] = 0ull; }
				continue;
			}
		} else {
			const uint64_t neutral = g.op == kMaskAnd ? 0ull : ~0ull; // the word that q cannot change
			prior                  = lane < 16u ? mw[lane] : neutral;
			if (ballot64(prior != neutral) == 0ull) { continue; } // AND of all zeros, OR of all ones: these 128 bytes were all that was read
			if (outside) {
				if (g.op == kMaskAnd && lane < 16u) { mw[lane] = 0ull; }
				continue;
			}
		}
		uint32_t p_begin, p_end;
		range_share(g.first, g.end, r0, p_begin, p_end);

		// 2. the part [j0, j1) of the list that the vector's zone record admits: all of it without a record or with a NaN bound
		uint32_t j0 = 0u, j1 = g.n_list;
		if (g.zones != nullptr && g.n_list > 0u) { sorted_list_zone<VB, GLOBAL>(s_list, list, g, v, j0, j1); }
		if (j1 <= j0) { // no element can be a member here (an empty list included): the descriptor is not read
			const uint64_t q = g.negate ? range_word(lane, p_begin, p_end) : 0ull;
			if (lane < 16u && !(g.op == kMaskOr && !g.negate)) { mw[lane] = g.op == kMaskAnd ? (prior & q) : g.op == kMaskOr ? (prior | q) : q; }
			continue;
		}

		// 3. the descriptor, the dictionary and the exception mask
		const DecodeVec<VB> V = decode_vec_load<VB>(c, v);
		exception_mask(V, s_exc, wave, lane);

		uint32_t before_exc = 0; // exceptions of the steps done
		uint64_t keep       = 0; // lane m < 16 keeps step m's ballot
		for (uint32_t b = 0; b < 16u; b += kStepBatch) {
			// 4. every load of kStepBatch steps is requested before the first is used
			StepBatch<VB, kStepBatch> R;
			step_request(V, s_exc[wave], b, lane, before_exc, R);
			T x[kStepBatch];
#pragma unroll
			for (uint32_t i = 0; i < kStepBatch; ++i) { x[i] = step_value(V, R, b, i, lane); }
			// 5. the batch's lower bounds, searched together, then one == each: -0.0 == 0.0; a NaN (value or element) is never a member
			uint32_t at[kStepBatch];
			in_list_search<VB, GLOBAL, kStepBatch>(s_list, list, g, j0, j1, x, 0u, at);
			T e[kStepBatch];
#pragma unroll
			for (uint32_t i = 0; i < kStepBatch; ++i) { e[i] = sorted_list_at<VB, GLOBAL>(s_list, list, g, at[i]); }
#pragma unroll
			for (uint32_t i = 0; i < kStepBatch; ++i) {
				const uint32_t m      = b + i;
				const uint32_t p      = 64u * m + lane;
				const bool     member = at[i] < j1 && e[i] == x[i];
				const uint64_t sel    = ballot64(p - p_begin < p_end - p_begin && member != (g.negate != 0)); // p_begin <= p < p_end
				keep                  = lane == m ? sel : keep;
			}
		}
		if (lane < 16u) { mw[lane] = g.op == kMaskAnd ? (prior & keep) : g.op == kMaskOr ? (prior | keep) : keep; } // one run of 128 bytes
	}
}

template <int VB>
static int launch_in_list_vb(hipStream_t stream, const ColumnStreams& c, const InArgs& args, unsigned grid) {
	if (args.stride > 1u) {
		hipLaunchKernelGGL((k_in_list<VB, true>), dim3(grid), dim3(kInThreads), 0, stream, c, args);
	} else {
		hipLaunchKernelGGL((k_in_list<VB, false>), dim3(grid), dim3(kInThreads), 0, stream, c, args);
	}
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

// col->n_vectors > 0, n > 0, n_list <= 2^31 - 1; range, op and alignments checked by the caller
int launch_select_in_mask(hipStream_t stream, const alpgpu_column* col, uint64_t first, uint64_t n, const void* d_list, uint64_t n_list, int negate, const void* d_zones, int op,
                          uint64_t* d_mask, int value_bytes, int n_cus) {
	const uint64_t    end     = first + n;
	const ListStaging staging = list_staging(n_list, value_bytes);
	InArgs            args {};
	args.v0      = op == kMaskOr ? first >> 10 : 0ull; // SET and AND cover every vector, OR those of the range
	args.n_range = op == kMaskOr ? ((end - 1) >> 10) - args.v0 + 1 : col->n_vectors;
	args.first   = first;
	args.end     = end;
	args.mask    = d_mask;
	args.list    = d_list;
	args.zones   = d_zones;
	args.n_list  = static_cast<uint32_t>(n_list);
	args.stride  = staging.stride;
	args.n_piv   = staging.n_piv;
	args.op      = op;
	args.negate  = negate != 0;
	const ColumnStreams c    = column_streams(col);
	const unsigned      grid = persistent_grid(args.n_range, kInWaves, n_cus, kInWgPerCu); // sized to the device: a workgroup stages the list once
	return value_bytes == 8 ? launch_in_list_vb<8>(stream, c, args, grid) : launch_in_list_vb<4>(stream, c, args, grid);
}

} // namespace alpgpu
