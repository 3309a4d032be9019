// group_device.hpp — grouped aggregation (include/alpgpu.h, "grouped aggregation": alpgpu_decode_group_sum_*): k_group.  Vector v of the VALUE
// column and vector v of the KEY column are decoded in registers side by side (register_decode.hpp: kStepBatch steps of both at a time, as k_pair
// decodes its pair); every group's range predicate on the key is then settled in that one pass, so that SUM and COUNT of G groups cost two
// decodes and not 2 G.
#pragma once
#include "register_decode.hpp"

namespace alpgpu {

// the groups' closed ranges in the key's own type: kernel arguments, wave-uniform.  The host pads the tier's unused groups with lo > hi.
template <int VB, int GT>
struct GroupBounds {
	static constexpr int      kTier = GT;
	typename DecodeVec<VB>::T lo[GT], hi[GT];
};
struct GroupArgs {
	uint64_t        n_vectors, wg_off; // the launch covers the whole column, this grid from workgroup wg_off on
	const uint64_t* mask;              // only read
	double*         sums;              // [n_groups][n_vectors]
	uint32_t*       counts;            // the same shape, nullable
	uint32_t        n_groups;          // rows stored: <= GT
};

// One wavefront per vector pair, four per workgroup, sharing nothing.  GT: the accumulator tier, so that acc[] and n[] are registers under
// full unrolling and never an indexed array.  Row g of the output is, bit for bit, what alpgpu_decode_sum_masked_* writes under the bitmap ANDed
// with alpgpu_select_mask_*(key, lo[g], hi[g]): the same lanes, the same m ascending, `acc + x` only where the value is selected, the same tree.
template <int VB, int GT>
__global__ __launch_bounds__(kSelThreads) void k_group(const ColumnStreams cv, const ColumnStreams ck, const GroupArgs g, const GroupBounds<VB, GT> r) {
	__shared__ uint64_t s_exc[kSelWaves][2][16]; // per wavefront and column: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t v    = (g.wg_off + blockIdx.x) * kSelWaves + wave;
	if (v >= g.n_vectors) { return; }

	// 1. the vector's 128 bytes of bitmap, lane m < 16 holding word m; without a set bit every group gets +0.0 and 0 and neither column is read
	uint64_t prior;
	if (!bitmap_words(g.mask, v, lane, prior)) {
		if (lane < g.n_groups) {
			g.sums[static_cast<uint64_t>(lane) * g.n_vectors + v] = 0.0;
			if (g.counts != nullptr) { g.counts[static_cast<uint64_t>(lane) * g.n_vectors + v] = 0u; }
		}
		return;
	}

	// 2. both descriptors and dictionaries, 3. both exception masks
	const DecodeVec<VB> A = decode_vec_load<VB>(cv, v);
	const DecodeVec<VB> B = decode_vec_load<VB>(ck, v);
	exception_masks(A, B, s_exc, wave, lane);

	uint32_t exc_a = 0, exc_b = 0; // exceptions of the steps done
	double   acc[GT];              // this lane's partial of every group
	uint32_t n[GT];                // wave-uniform: selected values of the steps done
#pragma unroll
	for (int j = 0; j < GT; ++j) {
		acc[j] = 0.0;
		n[j]   = 0u;
	}
	for (uint32_t b = 0; b < 16u; b += kStepBatch) {
		// 4. every load of kStepBatch steps of BOTH vectors is requested before the first is used
		StepBatch<VB, kStepBatch> Ra, Rb;
		step_request(A, s_exc[wave][0], b, lane, exc_a, Ra);
		step_request(B, s_exc[wave][1], b, lane, exc_b, Rb);
		// 5. the batch's values and their keys
		double                    x[kStepBatch];
		typename DecodeVec<VB>::T k[kStepBatch];
		bool                      bit[kStepBatch];
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			x[i]   = static_cast<double>(step_value(A, Ra, b, i, lane));
			k[i]   = step_value(B, Rb, b, i, lane);
			bit[i] = (readlane64(prior, b + i) >> lane) & 1ull;
		}
		// 6. every group, its bounds fetched once for the batch's steps (m ascending within the group: the documented order): NaN (key or bound)
		// never qualifies; -0.0 == 0.0; lo > hi selects nothing
#pragma unroll
		for (int j = 0; j < GT; ++j) {
#pragma unroll
			for (uint32_t i = 0; i < kStepBatch; ++i) {
				const bool q = bit[i] && k[i] >= r.lo[j] && k[i] <= r.hi[j];
				acc[j]       = q ? acc[j] + x[i] : acc[j]; // (an addition alone: nothing to contract)
				n[j] += static_cast<uint32_t>(__builtin_popcountll(ballot64(q)));
			}
		}
	}
	// 7. one tree per stored group; lane 0 stores
#pragma unroll
	for (int j = 0; j < GT; ++j) {
		if (static_cast<uint32_t>(j) < g.n_groups) {
			const double total = wave_tree_sum_f64(acc[j]);
			if (lane == 0u) {
				g.sums[static_cast<uint64_t>(j) * g.n_vectors + v] = total;
				if (g.counts != nullptr) { g.counts[static_cast<uint64_t>(j) * g.n_vectors + v] = n[j]; }
			}
		}
	}
}

// Host side, for k_group and k_group_minmax: the bounds of the smallest tier GT = 4, 8 or 16 that holds n_groups, in the key's own type (a float entry
// point's bounds are floats: they pass through double unchanged), the tier's unused groups padded with lo = 1 > hi = 0.  launch(bounds) launches the
// kernel of decltype(bounds)::kTier and returns the call's result.
template <int VB, class Launch>
inline int with_group_tier(const double* lo, const double* hi, uint32_t n_groups, Launch&& launch) {
	typedef typename DecodeVec<VB>::T T;
	const auto tier = [&](auto r) {
		for (uint32_t j = 0; j < static_cast<uint32_t>(decltype(r)::kTier); ++j) {
			r.lo[j] = j < n_groups ? static_cast<T>(lo[j]) : static_cast<T>(1);
			r.hi[j] = j < n_groups ? static_cast<T>(hi[j]) : static_cast<T>(0);
		}
		return launch(r);
	};
	return n_groups <= 4u ? tier(GroupBounds<VB, 4> {}) : n_groups <= 8u ? tier(GroupBounds<VB, 8> {}) : tier(GroupBounds<VB, 16> {});
}

} // namespace alpgpu
