// bucket_kernels.hip — bucketed aggregation (include/alpgpu.h, "bucketed aggregation": alpgpu_decode_bucket_sum_* / alpgpu_decode_bucket_minmax_*): SUM,
// the record {min, max} and the COUNT of a value column per bucket of a key column by sorted edges, both columns decoded side by side in registers, no
// decoded value reaching HBM.  It is k_histogram's bucket search (lds_bound over the edges staged in LDS, `upper` chosen by `right`) and its one-bucket
// zone rule put in front of the two keyed tables: k_keyed_sum's private per-wavefront tables in their documented order (keyed_kernels.hip) and
// k_keyed_minmax's one table per workgroup on LDS integer atomics (keyed_minmax_kernels.hip).
//
//   k_bucket_sum<VB, KCAP, WAVES>
//                         k_keyed_sum's skeleton: persistent workgroups, the edges staged into LDS behind ONE barrier, stripes taken by an integer
//                         ticket, a PRIVATE table per wavefront of n_edges + 1 doubles and 32-bit counts, the partials stored to row s of the scratch
//                         by plain vector stores; then k_keyed_reduce's tree over the S rows (k_keyed_init and k_keyed_reduce are keyed_kernels.hip's,
//                         declared in keyed_table.hpp).
//   k_bucket_minmax<VB, WAVES>
//                         k_keyed_minmax's skeleton: one table per workgroup (mn, mx, cnt), atomic_min_value / atomic_max_value on the value's bits
//                         behind the read-before-atomic guard, the 32-bit counts flushed every kKmmFlushEvery trips, a join by global integer atomics
//                         at the end; no scratch and no reduce kernel.  cnt[n_edges + 1] takes the rows whose key is a NaN.
//   a step                64 values of both columns.  Lane l searches its key's bucket: lds_bound over the edges [j0, j1) with upper = right ? 0 : ~0u,
//                         clamped to n_edges.  The step's members are m = w & ~ballot(key is a NaN): every key that is no NaN has a bucket.  From
//                         there the step is keyed_step / kmm_step unchanged (agree-on-one-bucket fast path, lone-lane shortcut, then bucket by bucket
//                         in first-lane order; guarded atomics for the records).
//   zones                 histogram's rules, not keyed's: the key vector's record {min, max} (no NaNs) is searched by the whole wavefront,
//                         a = bucket(min), b = bucket(max).  a <= b narrows the per-value search to the edges [a, b).  a == b on a key vector that is
//                         ALP without exceptions (only there a NaN is always an exception): every selected row has bucket a, the key vector's packed
//                         words are not requested and only the value vector is decoded.  b < a (a record that lies) and a NaN bound prune nothing.
//                         There is no "admits no key" class: word 2 of the trace stays 0.
//
// The steps (keyed_step, kmm_step), kmm_join, order_key, kmm_counts_flush, the tiers and the declarations of k_keyed_init / k_keyed_reduce are
// keyed_table.hpp's, the ones the keyed kernels use; the move was checked against the device assembly (profiles/r29_keyed_tables.txt).  The vector
// functions and kernel bodies stay this file's: as templates shared with the keyed kernels they compiled differently and k_bucket_sum ran behind.
//
// LDS: the edges take the keys' array, so the budget is k_keyed_sum's / k_keyed_minmax's.  HBM traffic per vector: theirs.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; launch bounds 512 and 768):
//   k_bucket_sum<8,  256,  8>   125 VGPRs,  28672 B LDS, 4 waves per SIMD, no scratch (67 SGPRs kept in VGPR lanes)
//   k_bucket_sum<8, 1024, 12>   130 VGPRs, 158720 B LDS, 3 waves per SIMD, no scratch (66 SGPRs kept in VGPR lanes)
//   k_bucket_sum<4,  256,  8>   103 VGPRs,  27648 B LDS, 4 waves per SIMD, no scratch (59 SGPRs kept in VGPR lanes)
//   k_bucket_sum<4, 1024, 12>   103 VGPRs, 154624 B LDS, 3 waves per SIMD, no scratch (62 SGPRs kept in VGPR lanes)
//   k_bucket_minmax<8, 8>       124 VGPRs,  30736 B LDS, 4 waves per SIMD, no scratch (70 SGPRs kept in VGPR lanes)
//   k_bucket_minmax<4, 8>       102 VGPRs,  18448 B LDS, 4 waves per SIMD, no scratch (67 SGPRs kept in VGPR lanes)
// Every instantiation runs at its keyed sibling's occupancy (k_keyed_sum 4 / 3, k_keyed_minmax 4 / 4), and that is asked for, not found: left to
// itself the compiler takes 131 VGPRs for k_bucket_sum<8, 256, 8> and 132 for k_bucket_minmax<8, 8> (the argument record is one word longer than the
// keyed ones and the NaN ballot is a second mask per step), which is 3 waves per SIMD, one workgroup per CU fewer than the grid is sized for.
// amdgpu_waves_per_eu(4) on the 8-wavefront kernels holds it to 128 registers; it meets that without scratch (the lines above).  The 12-wavefront
// tier is bound by its LDS to one workgroup per CU = 3 waves per SIMD, where 130 registers cost nothing, and asks for 3.
#include "keyed_table.hpp"

namespace alpgpu {

struct BucketArgs {
	uint64_t        n_vectors;
	uint64_t        stripe_vectors; // L                                      (SUM)
	uint32_t        n_stripes;      // S = ceil(n_vectors / L)                (SUM)
	uint32_t        n_edges;        // 0 .. ALPGPU_BUCKET_EDGES_MAX
	uint32_t        upper;          // lds_bound's mask: right ? 0 : ~0u
	const uint64_t* mask;           // nullable: every row
	const void*     edges;          // n_edges sorted elements of the key column's type
	const void*     zones;          // nullable: one record {min, max} per key vector
	uint32_t*       ticket;         // the scratch's header: the next stripe  (SUM)
	double*         partials;       // [S][n_edges + 1]                       (SUM)
	void*           out;            // n_edges + 1 records, joined into       (MIN / MAX)
	uint64_t*       counts;         // nullable: n_edges + 2 words, added to
	uint64_t*       trace;          // nullable: 4 words, added to
};

// The key vector's zone record into [j0, j1] (wave-uniform; histogram's rule).  True: both bounds lie in the one bucket j0.
template <class T>
__device__ __forceinline__ bool bucket_zone(const T* s_edges, const BucketArgs& g, uint64_t v, uint32_t& j0, uint32_t& j1) {
	const T* zone = static_cast<const T*>(g.zones) + 2 * v; // (wave-uniform)
	const T  z[2] = {zone[0], zone[1]};
	if (z[0] == z[0] && z[1] == z[1]) {
		uint32_t j[2];
		lds_bound<T, 2>(s_edges, g.n_edges > 0u ? g.n_edges - 1u : 0u, 0u, g.n_edges, z, g.upper, j); // the buckets of min and of max
		const uint32_t a = __builtin_amdgcn_readfirstlane(j[0]), b = __builtin_amdgcn_readfirstlane(j[1]);
		if (a <= b) {
			j0 = a;
			j1 = b;
			return a == b;
		}
	}
	return false;
}

// ---- SUM -------------------------------------------------------------------------------------------------------------------------------------------

// One vector pair by one wavefront.  Returns the class of the trace it fell into; nan_rows (wave-uniform) takes the selected rows whose key is a NaN.
template <int VB, int WAVES>
__device__ __forceinline__ uint32_t bucket_sum_vector(const ColumnStreams& cv, const ColumnStreams& ck, const BucketArgs& g, uint64_t v, uint32_t wave, uint32_t lane,
                                                      const typename DecodeVec<VB>::T* s_edges, double* s_sums, uint32_t* s_cnt, uint64_t (&s_exc)[WAVES][2][16], uint32_t& nan_rows) {
	typedef typename DecodeVec<VB>::T T;
	// 1. the selected bits, lane m < 16 holding word m
	uint64_t sel;
	if (!selected_words(g.mask, 0ull, g.n_vectors << 10, v, lane, sel)) { return kVectorSkipZero; }

	// 2. the part [j0, j1) of the edges that the key vector's zone record admits: all of them without a record, with a NaN bound or with min above max
	const uint32_t last_edge = g.n_edges > 0u ? g.n_edges - 1u : 0u;
	uint32_t       j0 = 0u, j1 = g.n_edges;
	if (g.zones != nullptr) {
		if (bucket_zone<T>(s_edges, g, v, j0, j1) && alp_without_exceptions(ck.descs[v])) { // no NaN can hide here: every selected row has bucket j0; the value vector alone is decoded
			const DecodeVec<VB> A = decode_vec_load<VB>(cv, v);
			if (A.cnt > 0) {
				if (lane < 16u) { s_exc[wave][0][lane] = 0ull; }
				wave_lds_sync();
				mark_exceptions<VB>(A, s_exc[wave][0], lane);
				wave_lds_sync();
			}
			uint32_t exc_a = 0, n_rows = 0;
			double   acc = 0.0; // lane 0's: the bucket's accumulator, read once and written once (no other bucket is touched in between)
			if (lane == 0u) { acc = s_sums[j0]; }
			for (uint32_t b = 0; b < 16u; b += kStepBatch) {
				StepBatch<VB, kStepBatch> Ra;
				step_request(A, s_exc[wave][0], b, lane, exc_a, Ra);
#pragma unroll
				for (uint32_t i = 0; i < kStepBatch; ++i) {
					const double   x = static_cast<double>(step_value(A, Ra, b, i, lane));
					const uint64_t w = readlane64(sel, b + i);
					if (w != 0ull) {
						acc += wave_tree_sum_f64(((w >> lane) & 1ull) ? x : 0.0);
						n_rows += static_cast<uint32_t>(__builtin_popcountll(w));
					}
				}
			}
			if (lane == 0u) {
				s_sums[j0] = acc;
				s_cnt[j0] += n_rows;
			}
			wave_lds_sync();
			return kVectorOneEntry;
		}
	}

	// 3. both descriptors and dictionaries, both exception masks
	const DecodeVec<VB> A = decode_vec_load<VB>(cv, v);
	const DecodeVec<VB> B = decode_vec_load<VB>(ck, v);
	exception_masks(A, B, s_exc, wave, lane);

	uint32_t exc_a = 0, exc_b = 0; // exceptions of the steps done
	for (uint32_t b = 0; b < 16u; b += kStepBatch) {
		// 4. every load of kStepBatch steps of BOTH vectors is requested before the first is used
		StepBatch<VB, kStepBatch> Ra, Rb;
		step_request(A, s_exc[wave][0], b, lane, exc_a, Ra);
		step_request(B, s_exc[wave][1], b, lane, exc_b, Rb);
		T      k[kStepBatch];
		double x[kStepBatch];
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			x[i] = static_cast<double>(step_value(A, Ra, b, i, lane));
			k[i] = step_value(B, Rb, b, i, lane);
		}
		// 5. the batch's buckets, searched together; the result lies in [j0, j1] whatever the edges hold and is clamped to the table
		uint32_t at[kStepBatch];
		lds_bound<T, kStepBatch>(s_edges, last_edge, j0, j1, k, g.upper, at);
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			const uint32_t idx  = at[i] < g.n_edges ? at[i] : g.n_edges;
			const uint64_t w    = readlane64(sel, b + i);
			const uint64_t nans = ballot64(!(k[i] == k[i]));
			nan_rows += static_cast<uint32_t>(__builtin_popcountll(w & nans));
			keyed_step(s_sums, s_cnt, w & ~nans, idx, x[i], lane);
		}
	}
	return kVectorDecoded;
}

template <int VB, uint32_t KCAP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(WAVES == kKeyedLargeWaves ? 3 : 4))) void k_bucket_sum(const ColumnStreams cv, const ColumnStreams ck, const BucketArgs g) {
	typedef typename DecodeVec<VB>::T T;
	__shared__ double   s_sums[WAVES][KCAP]; // per wavefront: the stripe's partials
	__shared__ uint32_t s_cnt[WAVES][KCAP];  // ... and counts
	__shared__ T        s_edges[KCAP];       // n_edges <= KCAP - 1 of them
	__shared__ uint64_t s_exc[WAVES][2][16]; // per wavefront and column: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t n_buckets = g.n_edges + 1u; // <= KCAP

	// 0. the edges into LDS, once per workgroup; the one barrier
	const T* edges = static_cast<const T*>(g.edges);
	for (uint32_t i = threadIdx.x; i < g.n_edges; i += 64u * WAVES) { s_edges[i] = edges[i]; }
	__syncthreads();

	double*   sums = s_sums[wave];
	uint32_t* cnt  = s_cnt[wave];
	uint32_t  did[4] = {0u, 0u, 0u, 0u};
	while (true) {
		// 1. a stripe by ticket
		uint32_t s = 0u;
		if (lane == 0u) { s = atomicAdd(g.ticket, 1u); }
		s = __builtin_amdgcn_readfirstlane(s);
		if (s >= g.n_stripes) { break; }
		// 2. the table zeroed
		for (uint32_t i = lane; i < n_buckets; i += 64u) {
			sums[i] = 0.0;
			cnt[i]  = 0u;
		}
		wave_lds_sync();
		// 3. the stripe's vectors, ascending
		const uint64_t v0 = static_cast<uint64_t>(s) * g.stripe_vectors;
		const uint64_t v1 = v0 + g.stripe_vectors < g.n_vectors ? v0 + g.stripe_vectors : g.n_vectors;
		uint32_t       nan_rows = 0u;
		for (uint64_t v = v0; v < v1; ++v) {
			const uint32_t what = bucket_sum_vector<VB, WAVES>(cv, ck, g, v, wave, lane, s_edges, sums, cnt, s_exc, nan_rows);
#pragma unroll
			for (uint32_t i = 0; i < 4u; ++i) { did[i] += what == i ? 1u : 0u; }
		}
		wave_lds_sync();
		// 4. the partials into row s of the scratch, 5. the counts into the call's
		double* row = g.partials + static_cast<uint64_t>(s) * n_buckets;
		for (uint32_t i = lane; i < n_buckets; i += 64u) {
			row[i] = sums[i];
			if (g.counts != nullptr) {
				const uint32_t n = cnt[i];
				if (n != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(g.counts) + i, static_cast<unsigned long long>(n)); }
			}
		}
		if (g.counts != nullptr && nan_rows != 0u && lane == 0u) {
			atomicAdd(reinterpret_cast<unsigned long long*>(g.counts) + n_buckets, static_cast<unsigned long long>(nan_rows));
		}
		wave_lds_sync();
	}
	if (g.trace != nullptr && lane < 4u) { // the trace: one add per wavefront and counter
		const uint32_t mine = lane == 0u ? did[0] : lane == 1u ? did[1] : lane == 2u ? did[2] : did[3];
		if (mine != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(g.trace) + lane, static_cast<unsigned long long>(mine)); }
	}
}

// ---- MIN / MAX -------------------------------------------------------------------------------------------------------------------------------------

// One vector pair by one wavefront.  Returns the class of the trace it fell into.  s_cnt[n_edges + 1] takes the selected rows whose key is a NaN.
template <int VB>
__device__ __forceinline__ uint32_t bucket_mm_vector(const ColumnStreams& cv, const ColumnStreams& ck, const BucketArgs& g, uint64_t v, uint32_t wave, uint32_t lane,
                                                     const typename DecodeVec<VB>::T* s_edges, typename DecodeVec<VB>::T* s_mn, typename DecodeVec<VB>::T* s_mx, uint32_t* s_cnt,
                                                     uint64_t (&s_exc)[kKmmWaves][2][16]) {
	typedef typename DecodeVec<VB>::T T;
	const bool counted = g.counts != nullptr;
	// 1. the selected bits, lane m < 16 holding word m
	uint64_t sel;
	if (!selected_words(g.mask, 0ull, g.n_vectors << 10, v, lane, sel)) { return kVectorSkipZero; }

	// 2. the part [j0, j1) of the edges that the key vector's zone record admits
	const uint32_t last_edge = g.n_edges > 0u ? g.n_edges - 1u : 0u;
	uint32_t       j0 = 0u, j1 = g.n_edges;
	if (g.zones != nullptr) {
		if (bucket_zone<T>(s_edges, g, v, j0, j1) && alp_without_exceptions(ck.descs[v])) { // every selected row has bucket j0; the value vector alone is decoded
			const DecodeVec<VB> A = decode_vec_load<VB>(cv, v);
			if (A.cnt > 0) {
				if (lane < 16u) { s_exc[wave][0][lane] = 0ull; }
				wave_lds_sync();
				mark_exceptions<VB>(A, s_exc[wave][0], lane);
				wave_lds_sync();
			}
			uint32_t exc_a = 0, n_rows = 0;
			T        mn = pos_inf<T>(), mx = -pos_inf<T>(); // this lane's, over the 16 steps
			for (uint32_t b = 0; b < 16u; b += kStepBatch) {
				StepBatch<VB, kStepBatch> Ra;
				step_request(A, s_exc[wave][0], b, lane, exc_a, Ra);
#pragma unroll
				for (uint32_t i = 0; i < kStepBatch; ++i) {
					const T        q = minmax_canonical(step_value(A, Ra, b, i, lane));
					const uint64_t w = readlane64(sel, b + i);
					minmax_feed(mn, mx, (w >> lane) & 1ull ? q : minmax_skip<T>());
					n_rows += static_cast<uint32_t>(__builtin_popcountll(w));
				}
			}
			wave_minmax<T>(mn, mx);
			kmm_join(s_mn, s_mx, j0, mn, mx, lane);
			if (counted && lane == 0u) { atomicAdd(&s_cnt[j0], n_rows); }
			return kVectorOneEntry;
		}
	}

	// 3. both descriptors and dictionaries, both exception masks
	const DecodeVec<VB> A = decode_vec_load<VB>(cv, v);
	const DecodeVec<VB> B = decode_vec_load<VB>(ck, v);
	exception_masks(A, B, s_exc, wave, lane);

	uint32_t exc_a = 0, exc_b = 0; // exceptions of the steps done
	uint32_t nan_rows = 0u;        // wave-uniform
	for (uint32_t b = 0; b < 16u; b += kStepBatch) {
		// 4. every load of kStepBatch steps of BOTH vectors is requested before the first is used
		StepBatch<VB, kStepBatch> Ra, Rb;
		step_request(A, s_exc[wave][0], b, lane, exc_a, Ra);
		step_request(B, s_exc[wave][1], b, lane, exc_b, Rb);
		T q[kStepBatch], k[kStepBatch];
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			q[i] = minmax_canonical(step_value(A, Ra, b, i, lane));
			k[i] = step_value(B, Rb, b, i, lane);
		}
		// 5. the batch's buckets, searched together; the result lies in [j0, j1] whatever the edges hold and is clamped to the table
		uint32_t at[kStepBatch];
		lds_bound<T, kStepBatch>(s_edges, last_edge, j0, j1, k, g.upper, at);
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			const uint32_t idx  = at[i] < g.n_edges ? at[i] : g.n_edges;
			const uint64_t w    = readlane64(sel, b + i);
			const uint64_t nans = ballot64(!(k[i] == k[i]));
			nan_rows += static_cast<uint32_t>(__builtin_popcountll(w & nans));
			kmm_step<T>(s_mn, s_mx, s_cnt, counted, w & ~nans, idx, q[i], lane);
		}
	}
	if (counted && nan_rows != 0u && lane == 0u) { atomicAdd(&s_cnt[g.n_edges + 1u], nan_rows); }
	return kVectorDecoded;
}

template <int VB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(4))) void k_bucket_minmax(const ColumnStreams cv, const ColumnStreams ck, const BucketArgs g) {
	typedef typename DecodeVec<VB>::T T;
	static_assert(WAVES == kKmmWaves, "the table's helpers are written for kKmmWaves");
	__shared__ T        s_mn[ALPGPU_KEYED_KEYS_MAX];
	__shared__ T        s_mx[ALPGPU_KEYED_KEYS_MAX];
	__shared__ T        s_edges[ALPGPU_KEYED_KEYS_MAX];
	__shared__ uint32_t s_cnt[ALPGPU_KEYED_KEYS_MAX + 1u];
	__shared__ uint64_t s_exc[WAVES][2][16]; // per wavefront and column: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t n_buckets = g.n_edges + 1u; // <= ALPGPU_KEYED_KEYS_MAX

	// 0. the edges into LDS and the table emptied, once per workgroup; the one barrier in front of the loop
	const T* edges = static_cast<const T*>(g.edges);
	for (uint32_t i = threadIdx.x; i < g.n_edges; i += 64u * WAVES) { s_edges[i] = edges[i]; }
	for (uint32_t i = threadIdx.x; i < n_buckets; i += 64u * WAVES) {
		s_mn[i] = pos_inf<T>();
		s_mx[i] = -pos_inf<T>();
	}
	for (uint32_t i = threadIdx.x; i <= n_buckets; i += 64u * WAVES) { s_cnt[i] = 0u; }
	__syncthreads();

	// every wavefront of the workgroup makes the same number of trips (the last may find no vector), so that the flush's barriers are met by all
	const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * WAVES;
	uint32_t       did[4]  = {0u, 0u, 0u, 0u};
	uint32_t       trips   = 0;
	for (uint64_t k0 = static_cast<uint64_t>(blockIdx.x) * WAVES; k0 < g.n_vectors; k0 += n_waves) {
		const uint64_t v = k0 + wave;
		if (v < g.n_vectors) {
			const uint32_t what = bucket_mm_vector<VB>(cv, ck, g, v, wave, lane, s_edges, s_mn, s_mx, s_cnt, s_exc);
#pragma unroll
			for (uint32_t i = 0; i < 4u; ++i) { did[i] += what == i ? 1u : 0u; }
		}
		if (++trips == kKmmFlushEvery) {
			trips = 0;
			if (g.counts != nullptr) { kmm_counts_flush(s_cnt, n_buckets + 1u, g.counts); }
		}
	}
	// the flush: the table's non-empty entries into the call's records, the counts into the call's
	__syncthreads();
	T* out = static_cast<T*>(g.out);
	for (uint32_t i = threadIdx.x; i < n_buckets; i += 64u * WAVES) {
		const T mn = s_mn[i], mx = s_mx[i];
		if (mn <= mx) {
			atomic_min_value(&out[2u * i], mn);
			atomic_max_value(&out[2u * i + 1u], mx);
		}
	}
	if (g.counts != nullptr) {
		for (uint32_t i = threadIdx.x; i <= n_buckets; i += 64u * WAVES) {
			const uint32_t c = s_cnt[i];
			if (c != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(g.counts) + i, static_cast<unsigned long long>(c)); }
		}
	}
	if (g.trace != nullptr && lane < 4u) { // the trace: one add per wavefront and counter
		const uint32_t mine = lane == 0u ? did[0] : lane == 1u ? did[1] : lane == 2u ? did[2] : did[3];
		if (mine != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(g.trace) + lane, static_cast<unsigned long long>(mine)); }
	}
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------------------

template <int VB>
static void bucket_sum_launch(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const BucketArgs& args, int n_cus, uint32_t grid_override) {
	const ColumnStreams cv = column_streams(val), ck = column_streams(key);
	if (args.n_edges + 1u <= kKeyedSmallKeys) {
		const unsigned grid = persistent_grid(args.n_stripes, kKeyedSmallWaves, n_cus, kKeyedSmallWgPerCu, 0, grid_override, kTuningGridMax);
		hipLaunchKernelGGL((k_bucket_sum<VB, kKeyedSmallKeys, kKeyedSmallWaves>), dim3(grid), dim3(64 * kKeyedSmallWaves), 0, stream, cv, ck, args);
	} else {
		const unsigned grid = persistent_grid(args.n_stripes, kKeyedLargeWaves, n_cus, kKeyedLargeWgPerCu, 0, grid_override, kTuningGridMax);
		hipLaunchKernelGGL((k_bucket_sum<VB, ALPGPU_KEYED_KEYS_MAX, kKeyedLargeWaves>), dim3(grid), dim3(64 * kKeyedLargeWaves), 0, stream, cv, ck, args);
	}
}

// val->n_vectors == key->n_vectors in 1 .. 2^32 - 1, n_edges <= ALPGPU_BUCKET_EDGES_MAX, the alignments checked by the caller; d_scratch: 64 bytes of
// header and keyed_stripes(n_vectors) rows of n_edges + 1 doubles.  The init, one launch of persistent workgroups, the reduce.
int launch_bucket_sum(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_edges, uint32_t n_edges,
                      int right, double* d_sums, uint64_t* d_counts, void* d_scratch, int value_bytes, int n_cus, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	BucketArgs args {};
	args.n_vectors      = val->n_vectors;
	args.stripe_vectors = keyed_stripe_vectors(val->n_vectors);
	args.n_stripes      = static_cast<uint32_t>(keyed_stripes(val->n_vectors));
	args.n_edges        = n_edges;
	args.upper          = right != 0 ? 0u : ~0u;
	args.mask           = d_mask;
	args.edges          = d_edges;
	args.zones          = d_zones;
	args.ticket         = static_cast<uint32_t*>(d_scratch);
	args.partials       = reinterpret_cast<double*>(static_cast<uint8_t*>(d_scratch) + 64);
	args.counts         = d_counts;
	args.trace          = d_trace;
	const uint32_t n_buckets = n_edges + 1u;
	hipLaunchKernelGGL(k_keyed_init, dim3((n_buckets + 1u + 255u) / 256u), dim3(256), 0, stream, d_counts, n_buckets + 1u, static_cast<uint64_t*>(d_scratch));
	if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	const uint32_t grid_override = tuning != nullptr ? tuning->grid : 0u;
	if (value_bytes == 8) {
		bucket_sum_launch<8>(stream, val, key, args, n_cus, grid_override);
	} else {
		bucket_sum_launch<4>(stream, val, key, args, n_cus, grid_override);
	}
	if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	hipLaunchKernelGGL(k_keyed_reduce, dim3(n_buckets), dim3(256), 0, stream, args.partials, args.n_stripes, n_buckets, d_sums);
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

// the same columns and edges, no scratch: launch_keyed_minmax_init over the n_edges + 1 records and n_edges + 2 counts, and one launch of persistent workgroups
int launch_bucket_minmax(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_edges, uint32_t n_edges,
                         int right, void* d_out, uint64_t* d_counts, int value_bytes, int n_cus, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	BucketArgs args {};
	args.n_vectors = val->n_vectors;
	args.n_edges   = n_edges;
	args.upper     = right != 0 ? 0u : ~0u;
	args.mask      = d_mask;
	args.edges     = d_edges;
	args.zones     = d_zones;
	args.out       = d_out;
	args.counts    = d_counts;
	args.trace     = d_trace;
	const int rc = launch_keyed_minmax_init(stream, d_out, d_counts, n_edges + 1u, value_bytes);
	if (rc != ALPGPU_OK) { return rc; }
	const unsigned      grid = persistent_grid(val->n_vectors, kKmmWaves, n_cus, kKmmWgPerCu, 0, tuning != nullptr ? tuning->grid : 0u, kTuningGridMax);
	const ColumnStreams cv = column_streams(val), ck = column_streams(key);
	if (value_bytes == 8) {
		hipLaunchKernelGGL((k_bucket_minmax<8, kKmmWaves>), dim3(grid), dim3(kKmmThreads), 0, stream, cv, ck, args);
	} else {
		hipLaunchKernelGGL((k_bucket_minmax<4, kKmmWaves>), dim3(grid), dim3(kKmmThreads), 0, stream, cv, ck, args);
	}
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

} // namespace alpgpu
