// join_kernels.hip — join probe (include/alpgpu.h, "join probe": alpgpu_join_probe_*): for every selected value of a compressed column, the position of
// its match in a sorted key list (or the build-side row id stored there) and the length of the equal run, compacted in index order.  The sorted
// list in LDS of k_in_list (sorted_list.hpp: staging, zone bounds, search and equality fetch are its functions) with the epilogue of k_select's TAKE arm.
//
//   k_join_probe<VB, GLOBAL, SPAN>   persistent workgroups of kInWaves wavefronts.  The workgroup stages the sorted keys (or, GLOBAL, every stride-th of
//                           them: the pivots) into 32 KiB of static LDS, passes ONE workgroup barrier and only then walks vectors v = wave_id,
//                           wave_id + n_waves, ...: every early-out sits behind that barrier.  Per vector: counts[v] (zero: done after 4 bytes),
//                           offsets[v] (at or behind the capacity: done), the 16 bitmap words, the zone check, then the decode in registers by
//                           register_decode.hpp in batches of kStepBatch steps.  A batch whose words are all zero requests nothing of the column and
//                           only moves the exception rank on, as TAKE does.  Without a bitmap counts[v] = 1024, offsets[v] = 1024 v and every word
//                           is all ones: nothing but the column is read.
//   the search              in_list_search (sorted_list.hpp): lb = the keys < x over [j0, j1), then one ==; SPAN: a second call with `upper` set,
//                           ub = the keys <= x, span = ub - lb.  A template flag and not a branch: the instances without a span keep lb's registers only.
//   the output slot         offsets[v] + the set bits of the words before + v_mbcnt of the value's own word: ascending, and no atomic anywhere.  The
//                           vector is left behind its last set bit or behind the capacity.
//   zones                   sorted_list_zone's two wave-uniform searches: j1 <= j0 (an empty list included) and every set bit of the vector gets NO_MATCH and
//                           span 0 from its bitmap words alone; else the per-value search runs over [j0, j1) only.
//
// HBM traffic per vector: with a bitmap the scan's 12 bytes and, where a bit is set below the capacity, the 128 bytes of bitmap; unless the zone record
// settles the vector, its descriptor, packed words and exception record (those only for the quarters of the vector that hold a bit); 8 (+ 4) (+ 8) bytes
// written per selected value; d_rows[lb] read per matched value; the keys once per workgroup.  One launch of at most 4 workgroups per CU.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; launch bounds 512 = 2 wavefronts per SIMD and workgroup):
//   k_join_probe<8, false, false>   76 VGPRs, 33792 B LDS, 6 waves per SIMD, no scratch
//   k_join_probe<8, false, true>    77 VGPRs, 33792 B LDS, 6 waves per SIMD, no scratch
//   k_join_probe<8, true, false>    79 VGPRs, 33792 B LDS, 6 waves per SIMD, no scratch (5 SGPRs kept in VGPR lanes)
//   k_join_probe<8, true, true>     88 VGPRs, 33792 B LDS, 5 waves per SIMD, no scratch (10 SGPRs kept in VGPR lanes)
//   k_join_probe<4, false, false>   66 VGPRs, 33792 B LDS, 7 waves per SIMD, no scratch
//   k_join_probe<4, false, true>    68 VGPRs, 33792 B LDS, 7 waves per SIMD, no scratch
//   k_join_probe<4, true, false>    67 VGPRs, 33792 B LDS, 7 waves per SIMD, no scratch (2 SGPRs kept in VGPR lanes)
//   k_join_probe<4, true, true>     75 VGPRs, 33792 B LDS, 6 waves per SIMD, no scratch (7 SGPRs kept in VGPR lanes)
// (33792 B of LDS: four workgroups per CU, as k_in_list.)
#include "select_device.hpp"
#include "sorted_list.hpp"

namespace alpgpu {

struct JoinArgs {
	uint64_t        n_vectors;
	const uint64_t* mask;     // nullable: every index
	const uint32_t* counts;   // [v], what k_mask_count wrote (not read without a bitmap)
	const uint64_t* offsets;  // [v], their exclusive prefix sum (not read without a bitmap)
	const int64_t*  rows;     // nullable: n_list payloads, read at matched positions only
	int64_t*        d_pos;
	uint32_t*       d_span;   // non-null exactly in the SPAN instances
	int64_t*        d_idx;    // nullable
	uint64_t        capacity; // > 0
	uint64_t*       d_count;  // non-null without a bitmap: takes n_vectors * 1024
};

template <int VB, bool GLOBAL, bool SPAN>
__global__ __launch_bounds__(kInThreads) void k_join_probe(const ColumnStreams c, const InArgs g, const JoinArgs a) {
	typedef typename DecodeVec<VB>::T T;
	__shared__ T        s_list[kInLdsBytes / VB];
	__shared__ uint64_t s_exc[kInWaves][16]; // per wavefront: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const T*       list = static_cast<const T*>(g.list);

	// 0. the keys (GLOBAL: their pivots) into LDS, once per workgroup; the one workgroup barrier of the kernel
	sorted_list_stage<VB, GLOBAL>(s_list, list, g);
	__syncthreads();
	if (a.d_count != nullptr && blockIdx.x == 0u && threadIdx.x == 0u) { *a.d_count = a.n_vectors << 10; } // no bitmap: the count is the column's length

	const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * kInWaves;
	for (uint64_t v = static_cast<uint64_t>(blockIdx.x) * kInWaves + wave; v < a.n_vectors; v += n_waves) {
		const uint64_t r0 = v << 10;

		// 1. the vector's set bits, its first output row and its 128 bytes of bitmap, lane m < 16 holding word m
		uint32_t total = 1024u;
		uint64_t out0  = r0;
		uint64_t prior = lane < 16u ? ~0ull : 0ull;
		if (a.mask != nullptr) {
			total = a.counts[v];
			if (total == 0u) { continue; } // a vector without a set bit costs these four bytes
			out0 = a.offsets[v];
		}
		if (out0 >= a.capacity) { continue; } // ... and one at or behind the capacity its offset too: its descriptor is not read
		if (a.mask != nullptr) { prior = lane < 16u ? a.mask[16ull * v + lane] : 0ull; } // one read of 128 bytes

		// 2. the part [j0, j1) of the keys that the vector's zone record admits: all of them without a record or with a NaN bound
		uint32_t j0 = 0u, j1 = g.n_list;
		if (g.zones != nullptr && g.n_list > 0u) { sorted_list_zone<VB, GLOBAL>(s_list, list, g, v, j0, j1); }
		uint32_t before_sel = 0; // set bits of the steps done (wave-uniform)
		if (j1 <= j0) { // no key can match here (an empty list included): the rows come from the bitmap words, the descriptor is not read
			for (uint32_t m = 0; m < 16u; ++m) {
				const uint64_t w = readlane64(prior, m);
				const uint64_t j = out0 + before_sel + mbcnt64(w, 0u);
				if (((w >> lane) & 1ull) && j < a.capacity) {
					a.d_pos[j] = ALPGPU_JOIN_NO_MATCH;
					if constexpr (SPAN) { a.d_span[j] = 0u; }
					if (a.d_idx != nullptr) { a.d_idx[j] = static_cast<int64_t>(r0 + 64u * m + lane); }
				}
				before_sel += static_cast<uint32_t>(__builtin_popcountll(w));
				if (before_sel >= total || out0 + before_sel >= a.capacity) { break; }
			}
			continue;
		}

		// 3. the descriptor, the dictionary and the exception mask
		const DecodeVec<VB> V = decode_vec_load<VB>(c, v);
		exception_mask(V, s_exc, wave, lane);

		uint32_t before_exc = 0; // exceptions of the steps done
		for (uint32_t b = 0; b < 16u; b += kStepBatch) {
			// no bit set in these kStepBatch words: nothing of the column is requested, but the exceptions of the steps passed over still count
			// towards the rank of those behind them
			if (ballot64(lane >= b && lane < b + kStepBatch && prior != 0ull) == 0ull) {
				if (V.cnt > 0) {
#pragma unroll
					for (uint32_t i = 0; i < kStepBatch; ++i) { before_exc += static_cast<uint32_t>(__builtin_popcountll(s_exc[wave][b + i])); } // (every lane reads the same word)
				}
				continue;
			}
			// 4. every load of kStepBatch steps is requested before the first is used
			StepBatch<VB, kStepBatch> R;
			step_request(V, s_exc[wave], b, lane, before_exc, R);
			T x[kStepBatch];
#pragma unroll
			for (uint32_t i = 0; i < kStepBatch; ++i) { x[i] = step_value(V, R, b, i, lane); }
			// 5. the batch's lower bounds, searched together, then one == each: -0.0 == 0.0; a NaN (value or key) never matches
			uint32_t lb[kStepBatch];
			in_list_search<VB, GLOBAL, kStepBatch>(s_list, list, g, j0, j1, x, 0u, lb);
			T e[kStepBatch];
#pragma unroll
			for (uint32_t i = 0; i < kStepBatch; ++i) { e[i] = sorted_list_at<VB, GLOBAL>(s_list, list, g, lb[i]); }
			uint32_t ub[kStepBatch];
			if constexpr (SPAN) { in_list_search<VB, GLOBAL, kStepBatch>(s_list, list, g, j0, j1, x, (1u << kStepBatch) - 1u, ub); }
			// 6. the rows of the batch's set bits
#pragma unroll
			for (uint32_t i = 0; i < kStepBatch; ++i) {
				const uint32_t m = b + i;
				const uint64_t w = readlane64(prior, m);
				const uint64_t j = out0 + before_sel + mbcnt64(w, 0u);
				if (((w >> lane) & 1ull) && j < a.capacity) { // (lanes of a dense word store side by side)
					const bool match = lb[i] < j1 && e[i] == x[i];
					int64_t    pos   = ALPGPU_JOIN_NO_MATCH;
					if (match) { pos = a.rows != nullptr ? a.rows[lb[i]] : static_cast<int64_t>(lb[i]); } // (lb < j1 <= n_list)
					a.d_pos[j] = pos;
					if constexpr (SPAN) { a.d_span[j] = ub[i] > lb[i] ? ub[i] - lb[i] : 0u; } // (both in [j0, j1]: at most n_list whatever the list holds)
					if (a.d_idx != nullptr) { a.d_idx[j] = static_cast<int64_t>(r0 + 64u * m + lane); }
				}
				before_sel += static_cast<uint32_t>(__builtin_popcountll(w));
			}
			if (before_sel >= total || out0 + before_sel >= a.capacity) { break; } // the vector's last set bit, or the capacity, is behind us
		}
	}
}

template <int VB, bool GLOBAL>
static void launch_join_span(hipStream_t stream, const ColumnStreams& c, const InArgs& g, const JoinArgs& a, unsigned grid) {
	if (a.d_span != nullptr) {
		hipLaunchKernelGGL((k_join_probe<VB, GLOBAL, true>), dim3(grid), dim3(kInThreads), 0, stream, c, g, a);
	} else {
		hipLaunchKernelGGL((k_join_probe<VB, GLOBAL, false>), dim3(grid), dim3(kInThreads), 0, stream, c, g, a);
	}
}
template <int VB>
static int launch_join_vb(hipStream_t stream, const ColumnStreams& c, const InArgs& g, const JoinArgs& a, unsigned grid) {
	if (g.stride > 1u) {
		launch_join_span<VB, true>(stream, c, g, a, grid);
	} else {
		launch_join_span<VB, false>(stream, c, g, a, grid);
	}
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

// col->n_vectors > 0, n_keys <= 2^31 - 1, d_pos non-null when capacity > 0; the alignments checked by the caller.  With a bitmap: the popcount pass and the
// scan of mask_kernels.hip, then (capacity > 0) the probe.  Without: the probe alone, which writes the count, or (capacity == 0) launch_fill_u64.
int launch_join_probe(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, const void* d_zones, const void* d_keys, uint64_t n_keys, const int64_t* d_rows,
                      int64_t* d_pos, uint32_t* d_span, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch, int value_bytes, int n_cus) {
	JoinArgs a {};
	if (d_mask != nullptr) {
		const SelScratch s  = select_scratch(d_scratch, col->n_vectors);
		const int        rc = launch_mask_count_scan(stream, d_mask, col->n_vectors, d_count, s);
		if (rc != ALPGPU_OK || capacity == 0) { return rc; }
		a.counts  = s.counts;
		a.offsets = s.offsets;
	} else {
		if (capacity == 0) { return launch_fill_u64(stream, d_count, 1u, col->n_vectors << 10); }
		a.d_count = d_count;
	}
	a.n_vectors = col->n_vectors;
	a.mask      = d_mask;
	a.rows      = d_rows;
	a.d_pos     = d_pos;
	a.d_span    = d_span;
	a.d_idx     = d_idx;
	a.capacity  = capacity;
	const ListStaging staging = list_staging(n_keys, value_bytes);
	InArgs            g {};
	g.list   = d_keys;
	g.zones  = d_zones;
	g.n_list = static_cast<uint32_t>(n_keys);
	g.stride = staging.stride;
	g.n_piv  = staging.n_piv;
	const ColumnStreams c    = column_streams(col);
	const unsigned      grid = persistent_grid(col->n_vectors, kInWaves, n_cus, kInWgPerCu); // sized to the device: a workgroup stages the keys once
	return value_bytes == 8 ? launch_join_vb<8>(stream, c, g, a, grid) : launch_join_vb<4>(stream, c, g, a, grid);
}

} // namespace alpgpu
