// minmax_device.hpp — masked and grouped MIN / MAX (include/alpgpu.h, "masked and grouped MIN / MAX": alpgpu_decode_minmax_masked_*,
// alpgpu_decode_group_minmax_*): k_minmax_masked and k_group_minmax, on the in-register decode of register_decode.hpp in batches of kStepBatch
// steps.  What they write are zone records (wave_minmax.hpp: NaNs ignored, -0.0 < +0.0, {+inf, -inf} for nothing) over the SELECTED values of
// a vector.  Minimum and maximum are exactly associative and commutative, so a record is a function of the selected values alone and no order
// needs documenting.
#pragma once
#include "group_device.hpp" // GroupBounds
#include "register_decode.hpp"
#include "wave_minmax.hpp"

namespace alpgpu {

struct MinmaxArgs {
	uint64_t        n_vectors, wg_off; // the launch covers the whole column, this grid from workgroup wg_off on
	const uint64_t* mask;              // only read
	void*           zones;             // masked: [n_vectors] records {min, max} of the column's type; grouped: [n_groups][n_vectors]
	uint32_t*       counts;            // the same shape, nullable
	uint32_t        n_groups;          // grouped: rows stored, <= GT
};

// a quiet NaN: what v_min / v_max skip (IEEE mode), so an unselected value fed as this changes neither accumulator
template <class T>
__device__ __forceinline__ T minmax_skip() {
	if constexpr (sizeof(T) == 8) { return __longlong_as_double(0x7FF8000000000000ll); } else { return __uint_as_float(0x7FC00000u); }
}
__device__ __forceinline__ double minmax_canonical(double x) { return fmax_num(x, x); } // minmax_take's first step: a signalling NaN quieted, anything else as it is
__device__ __forceinline__ float  minmax_canonical(float x) { return fmax_num_f32(x, x); }
__device__ __forceinline__ void   minmax_feed(double& mn, double& mx, double q) { // q canonical
	mn = fmin_num(mn, q);
	mx = fmax_num(mx, q);
}
__device__ __forceinline__ void minmax_feed(float& mn, float& mx, float q) {
	mn = fmin_num_f32(mn, q);
	mx = fmax_num_f32(mx, q);
}
// one record, one store of 16 (8) bytes
template <class T>
__device__ __forceinline__ void zone_store(void* zones, uint64_t i, T mn, T mx) {
	if constexpr (sizeof(T) == 8) { static_cast<double2*>(zones)[i] = make_double2(mn, mx); } else { static_cast<float2*>(zones)[i] = make_float2(mn, mx); }
}

// One wavefront per vector, four per workgroup, sharing nothing.  Under a full bitmap the record is that of alpgpu_zone_map_*.
template <int VB>
__global__ __launch_bounds__(kSelThreads) void k_minmax_masked(const ColumnStreams c, const MinmaxArgs g) {
	typedef typename DecodeVec<VB>::T T;
	__shared__ uint64_t             s_exc[kSelWaves][16]; // per wavefront: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t v    = (g.wg_off + blockIdx.x) * kSelWaves + wave;
	if (v >= g.n_vectors) { return; }

	// 1. the vector's 128 bytes of bitmap, lane m < 16 holding word m; without a set bit the record is empty and the column is not read
	uint64_t prior;
	if (!bitmap_words(g.mask, v, lane, prior)) {
		if (lane == 0u) {
			zone_store<T>(g.zones, v, pos_inf<T>(), -pos_inf<T>());
			if (g.counts != nullptr) { g.counts[v] = 0u; }
		}
		return;
	}

	// 2. the descriptor and dictionary, 3. the exception mask
	const DecodeVec<VB> A = decode_vec_load<VB>(c, v);
	exception_mask(A, s_exc, wave, lane);

	uint32_t exc_a = 0; // exceptions of the steps done
	uint32_t n_set = 0; // set bits of the steps done
	T        mn = pos_inf<T>(), mx = -pos_inf<T>();
	for (uint32_t b = 0; b < 16u; b += kStepBatch) {
		// 4. every load of kStepBatch steps is requested before the first is used
		StepBatch<VB, kStepBatch> Ra;
		step_request(A, s_exc[wave], b, lane, exc_a, Ra);
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			// 5. the value, taken or skipped by its bit: selected NaNs are counted and ignored
			const T        q = minmax_canonical(step_value(A, Ra, b, i, lane));
			const uint64_t w = readlane64(prior, b + i);
			minmax_feed(mn, mx, (w >> lane) & 1ull ? q : minmax_skip<T>());
			n_set += static_cast<uint32_t>(__builtin_popcountll(w));
		}
	}
	wave_minmax<T>(mn, mx);
	if (lane == 0u) {
		zone_store<T>(g.zones, v, mn, mx);
		if (g.counts != nullptr) { g.counts[v] = n_set; }
	}
}

// k_group's skeleton (group_device.hpp): one wavefront per vector pair, the groups' bounds as kernel arguments, the tier's unused groups padded
// with lo > hi, the counts wave-uniform from ballots.  GT: the accumulator tier, so that mn[], mx[] and n[] are registers under full unrolling
// and never an indexed array.  Row g of the output is what k_minmax_masked writes under the bitmap ANDed with
// alpgpu_select_mask_*(key, lo[g], hi[g]), and its counts are k_group's.
template <int VB, int GT>
__global__ __launch_bounds__(kSelThreads) void k_group_minmax(const ColumnStreams cv, const ColumnStreams ck, const MinmaxArgs g, const GroupBounds<VB, GT> r) {
	typedef typename DecodeVec<VB>::T T;
	__shared__ uint64_t             s_exc[kSelWaves][2][16]; // per wavefront and column: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t v    = (g.wg_off + blockIdx.x) * kSelWaves + wave;
	if (v >= g.n_vectors) { return; }

	// 1. the vector's 128 bytes of bitmap; without a set bit every group's record is empty and neither column is read
	uint64_t prior;
	if (!bitmap_words(g.mask, v, lane, prior)) {
		if (lane < g.n_groups) {
			zone_store<T>(g.zones, static_cast<uint64_t>(lane) * g.n_vectors + v, pos_inf<T>(), -pos_inf<T>());
			if (g.counts != nullptr) { g.counts[static_cast<uint64_t>(lane) * g.n_vectors + v] = 0u; }
		}
		return;
	}

	// 2. both descriptors and dictionaries, 3. both exception masks
	const DecodeVec<VB> A = decode_vec_load<VB>(cv, v);
	const DecodeVec<VB> B = decode_vec_load<VB>(ck, v);
	exception_masks(A, B, s_exc, wave, lane);

	uint32_t exc_a = 0, exc_b = 0; // exceptions of the steps done
	T        mn[GT], mx[GT];       // this lane's candidates of every group
	uint32_t n[GT];                // wave-uniform: selected values of the steps done
#pragma unroll
	for (int j = 0; j < GT; ++j) {
		mn[j] = pos_inf<T>();
		mx[j] = -pos_inf<T>();
		n[j]  = 0u;
	}
	for (uint32_t b = 0; b < 16u; b += kStepBatch) {
		// 4. every load of kStepBatch steps of BOTH vectors is requested before the first is used
		StepBatch<VB, kStepBatch> Ra, Rb;
		step_request(A, s_exc[wave][0], b, lane, exc_a, Ra);
		step_request(B, s_exc[wave][1], b, lane, exc_b, Rb);
		// 5. the batch's values, canonical once, and their keys
		T    q[kStepBatch], k[kStepBatch];
		bool bit[kStepBatch];
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			q[i]   = minmax_canonical(step_value(A, Ra, b, i, lane));
			k[i]   = step_value(B, Rb, b, i, lane);
			bit[i] = (readlane64(prior, b + i) >> lane) & 1ull;
		}
		// 6. every group (select_mask's predicate: a NaN key or bound never qualifies; -0.0 == 0.0; lo > hi selects nothing): an unselected value
		// goes in as a quiet NaN, which v_min / v_max skip
#pragma unroll
		for (int j = 0; j < GT; ++j) {
#pragma unroll
			for (uint32_t i = 0; i < kStepBatch; ++i) {
				const bool sel = bit[i] && k[i] >= r.lo[j] && k[i] <= r.hi[j];
				minmax_feed(mn[j], mx[j], sel ? q[i] : minmax_skip<T>());
				n[j] += static_cast<uint32_t>(__builtin_popcountll(ballot64(sel)));
			}
		}
	}
	// 7. one reduction per stored group; lane 0 stores
#pragma unroll
	for (int j = 0; j < GT; ++j) {
		if (static_cast<uint32_t>(j) < g.n_groups) {
			wave_minmax<T>(mn[j], mx[j]);
			if (lane == 0u) {
				zone_store<T>(g.zones, static_cast<uint64_t>(j) * g.n_vectors + v, mn[j], mx[j]);
				if (g.counts != nullptr) { g.counts[static_cast<uint64_t>(j) * g.n_vectors + v] = n[j]; }
			}
		}
	}
}

} // namespace alpgpu
