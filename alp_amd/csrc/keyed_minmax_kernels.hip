// keyed_minmax_kernels.hip — keyed MIN / MAX (include/alpgpu.h, "keyed MIN / MAX": alpgpu_decode_keyed_minmax_*): the record {min, max} and the COUNT of a
// value column per key of a sorted key list, the key column decoded beside it, no decoded value reaching HBM.  The parts are keyed_kernels.hip's (the
// side-by-side decode of register_decode.hpp, lds_bound over the staged keys, selected_words with the constant-vector predicate), k_histogram's
// skeleton (histogram_kernels.hip) and the records' order of wave_minmax.hpp.  The step (kmm_step, kmm_join, order_key), the count flush
// and the tiers are keyed_table.hpp's, shared with bucket_kernels.hip; the move was checked against the device assembly (profiles/r29_keyed_tables.txt).
//
//   k_keyed_minmax_init   {+inf, -inf} into the n_keys records and 0 into the n_keys + 1 counts: a kernel, no memset node (mask_kernels.hip says why).
//   k_keyed_minmax<VB, WAVES>
//                         persistent workgroups of WAVES wavefronts.  The workgroup stages the keys into LDS, fills ONE table for all its wavefronts
//                         (mn[i] = +inf, mx[i] = -inf, cnt[i] = 0), passes one barrier and then walks vectors v = wave id, wave id + waves, ...; every
//                         wavefront of a workgroup makes the same number of trips (the last may find no vector), so that the barriers of the flush are
//                         met by all, idle wavefronts included.  Minimum and maximum are exact and order-free, so no summation order has to be fixed:
//                         no private table per wavefront, no stripes, no scratch, no reduce kernel.
//   an update             an LDS integer atomic on the value's bits in the records' order (atomic_min_value / atomic_max_value: ds_min_i64 / ds_max_u64,
//                         ds_max_i64 / ds_min_u64, their 32-bit forms for float; no compare-and-swap loop).  A NaN value never reaches an atomic; it is
//                         counted only.
//   a step                64 values of both columns.  Lane l searches its key (lds_bound's lower bound, one ==).  m = the selected, matched lanes.
//                           all of m agree on one key     one wave_minmax (the other lanes fed minmax_skip), lane 0's two atomics if the step had a
//                                                         number, one count add of popcount(m);
//                           otherwise                     a lane reads its key's {mn, mx} with plain LDS loads and issues an atomic only where its
//                                                         value improves on what it read, compared by the records' INTEGER order key (C's < would drop
//                                                         a -0.0 that arrives behind +0.0).  A stale read is safe: the table moves one way, so a stale
//                                                         value can cause a needless atomic and never a missed one.  One LDS add per lane for the count.
//                         With d_counts == NULL no count is kept at all.
//   zones                 keyed_kernels.hip's rules: the key vector's record {min, max} (no NaNs) gives [j0, j1) = the keys it admits.  None: the
//                         selected bits are rows without a key, neither column is read.  min == max on a vector that is ALP without exceptions: every
//                         selected row has key j0; only the value vector is decoded, each lane keeps {mn, mx} over the 16 steps in registers, then one
//                         wave_minmax and one guarded pair of atomics.  Otherwise the per-value search is over [j0, j1).  Every probe index is clamped.
//   the flush             after a barrier thread i, i + threads, ... joins its non-empty entry into d_out[i] by global atomic_min_value /
//                         atomic_max_value and adds its count (and the rows without a key) by an integer atomic.  The 32-bit LDS counts are also
//                         flushed every kKmmFlushEvery trips (a trip adds at most WAVES x 1024 to one of them).  No workgroup waits for another.
//
// LDS banks: mn, mx and cnt are consecutive words, so 64 lanes with dense, distinct keys touch 64 neighbouring entries; equal keys meet in the atomic
// unit, which is what the guard keeps them from: once a key's record holds its range, its rows cost two loads and no atomic.
//
// HBM traffic per vector: the bitmap's 128 bytes (none with a NULL bitmap) and, unless they or the zone record settle the vector, both vectors'
// descriptors, packed words and exception records; the keys once per workgroup; 2 n_keys atomics per workgroup at its end.
//
// One capacity tier, 1 .. 1024 keys.  Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; launch bounds 512 = 2 wavefronts
// per SIMD and workgroup):
//   k_keyed_minmax<8, 8>   128 VGPRs, 30736 B LDS, 4 waves per SIMD, no scratch (47 SGPRs kept in VGPR lanes)
//   k_keyed_minmax<4, 8>   105 VGPRs, 18448 B LDS, 4 waves per SIMD, no scratch (49 SGPRs kept in VGPR lanes)
//   k_keyed_minmax_init    10 / 6 VGPRs (double / float), no LDS, no scratch
// WAVES = 8 and kKmmWgPerCu = 2: the registers admit 4 wavefronts per SIMD for both precisions (128 is the step's upper edge; the float kernel's 105
// is above the 96 that a fifth would take), which is 16 wavefronts per CU = two workgroups of 8; their LDS, 2 x 30 KiB, is far below the CU's 160 KiB
// and decides nothing.  One workgroup of 16 would hold the same wavefronts with half the staging, but puts 16 wavefronts on one table's atomics and
// one barrier; 4 wavefronts per workgroup would stage the keys and fill the table twice as often.  Both precisions take the same grid.
// The guard (read before atomic) is measured against unconditional atomics with -DALPGPU_KEYED_MINMAX_NO_GUARD (tools/time_keyed_minmax.py --ab); the
// bits are the same.
#include "keyed_table.hpp"

namespace alpgpu {

struct KeyedMinmaxArgs {
	uint64_t        n_vectors;
	const uint64_t* mask;   // nullable: every row
	const void*     keys;   // n_keys sorted elements of the columns' type
	const void*     zones;  // nullable: one record {min, max} per key vector
	void*           out;    // n_keys records {min, max} of the columns' type, joined into
	uint64_t*       counts; // nullable: n_keys + 1 words, added to
	uint64_t*       trace;  // nullable: 4 words, added to
	uint32_t        n_keys; // 1 .. ALPGPU_KEYED_KEYS_MAX
};

// One vector pair by one wavefront.  Returns the class of the trace it fell into.  s_cnt[n_keys] takes the selected rows without a key.
template <int VB>
__device__ __forceinline__ uint32_t kmm_vector(const ColumnStreams& cv, const ColumnStreams& ck, const KeyedMinmaxArgs& g, uint64_t v, uint32_t wave, uint32_t lane,
                                               const typename DecodeVec<VB>::T* s_keys, typename DecodeVec<VB>::T* s_mn, typename DecodeVec<VB>::T* s_mx, uint32_t* s_cnt,
                                               uint64_t (&s_exc)[kKmmWaves][2][16]) {
	typedef typename DecodeVec<VB>::T T;
	const bool counted = g.counts != nullptr;
	// 1. the selected bits, lane m < 16 holding word m
	uint64_t sel;
	if (!selected_words(g.mask, 0ull, g.n_vectors << 10, v, lane, sel)) { return kVectorSkipZero; }

	// 2. the part [j0, j1) of the keys that the key vector's zone record admits: all of them without a record or with a NaN bound
	const uint32_t last_key = g.n_keys - 1u;
	uint32_t       j0 = 0u, j1 = g.n_keys;
	if (g.zones != nullptr) {
		const T* zone = static_cast<const T*>(g.zones) + 2 * v; // (wave-uniform)
		const T  z[2] = {zone[0], zone[1]};
		if (z[0] == z[0] && z[1] == z[1]) {
			uint32_t j[2];
			lds_bound<T, 2>(s_keys, last_key, 0u, g.n_keys, z, 2u, j); // the first key >= min, the first key > max
			j0 = __builtin_amdgcn_readfirstlane(j[0]);
			j1 = __builtin_amdgcn_readfirstlane(j[1]);
			if (j1 <= j0) { // no key lies in the record: rows without a key
				if (counted) {
					const uint32_t n = selected_count(sel);
					if (lane == 63u) { atomicAdd(&s_cnt[g.n_keys], n); }
				}
				return kVectorNoEntry;
			}
			if (z[0] == z[1] && alp_without_exceptions(ck.descs[v])) { // no NaN can hide here: every selected row has key j0; the value vector alone is decoded
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
	}

	// 3. both descriptors and dictionaries, both exception masks
	const DecodeVec<VB> A = decode_vec_load<VB>(cv, v);
	const DecodeVec<VB> B = decode_vec_load<VB>(ck, v);
	exception_masks(A, B, s_exc, wave, lane);

	uint32_t exc_a = 0, exc_b = 0; // exceptions of the steps done
	uint32_t unmatched = 0u;       // wave-uniform
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
		// 5. the batch's keys, searched together: the lower bound and one ==.  A NaN key is never equal; the index read is clamped to the keys staged.
		uint32_t at[kStepBatch];
		lds_bound<T, kStepBatch>(s_keys, last_key, j0, j1, k, 0u, at);
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			const uint32_t idx = at[i] < last_key ? at[i] : last_key;
			const uint64_t w   = readlane64(sel, b + i);
			const uint64_t m   = w & ballot64(s_keys[idx] == k[i]);
			unmatched += static_cast<uint32_t>(__builtin_popcountll(w & ~m));
			kmm_step<T>(s_mn, s_mx, s_cnt, counted, m, idx, q[i], lane);
		}
	}
	if (counted && unmatched != 0u && lane == 0u) { atomicAdd(&s_cnt[g.n_keys], unmatched); }
	return kVectorDecoded;
}

template <class T>
__global__ __launch_bounds__(256) void k_keyed_minmax_init(T* out, uint32_t n_keys, uint64_t* counts) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < n_keys) {
		out[2u * i]      = pos_inf<T>();
		out[2u * i + 1u] = -pos_inf<T>();
	}
	if (counts != nullptr && i <= n_keys) { counts[i] = 0ull; }
}

template <int VB, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_keyed_minmax(const ColumnStreams cv, const ColumnStreams ck, const KeyedMinmaxArgs g) {
	typedef typename DecodeVec<VB>::T T;
	static_assert(WAVES == kKmmWaves, "the table's helpers are written for kKmmWaves");
	__shared__ T        s_mn[ALPGPU_KEYED_KEYS_MAX];
	__shared__ T        s_mx[ALPGPU_KEYED_KEYS_MAX];
	__shared__ T        s_keys[ALPGPU_KEYED_KEYS_MAX];
	__shared__ uint32_t s_cnt[ALPGPU_KEYED_KEYS_MAX + 1u];
	__shared__ uint64_t s_exc[WAVES][2][16]; // per wavefront and column: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;

	// 0. the keys into LDS and the table emptied, once per workgroup; the one barrier in front of the loop
	const T* keys = static_cast<const T*>(g.keys);
	for (uint32_t i = threadIdx.x; i < g.n_keys; i += 64u * WAVES) {
		s_keys[i] = keys[i];
		s_mn[i]   = pos_inf<T>();
		s_mx[i]   = -pos_inf<T>();
	}
	for (uint32_t i = threadIdx.x; i <= g.n_keys; i += 64u * WAVES) { s_cnt[i] = 0u; }
	__syncthreads();

	// every wavefront of the workgroup makes the same number of trips (the last may find no vector), so that the flush's barriers are met by all
	const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * WAVES;
	uint32_t       did[4]  = {0u, 0u, 0u, 0u};
	uint32_t       trips   = 0;
	for (uint64_t k0 = static_cast<uint64_t>(blockIdx.x) * WAVES; k0 < g.n_vectors; k0 += n_waves) {
		const uint64_t v = k0 + wave;
		if (v < g.n_vectors) {
			const uint32_t what = kmm_vector<VB>(cv, ck, g, v, wave, lane, s_keys, s_mn, s_mx, s_cnt, s_exc);
#pragma unroll
			for (uint32_t i = 0; i < 4u; ++i) { did[i] += what == i ? 1u : 0u; }
		}
		if (++trips == kKmmFlushEvery) {
			trips = 0;
			if (g.counts != nullptr) { kmm_counts_flush(s_cnt, g.n_keys + 1u, g.counts); }
		}
	}
	// the flush: the table's non-empty entries into the call's records, the counts into the call's
	__syncthreads();
	T* out = static_cast<T*>(g.out);
	for (uint32_t i = threadIdx.x; i < g.n_keys; i += 64u * WAVES) {
		const T mn = s_mn[i], mx = s_mx[i];
		if (mn <= mx) {
			atomic_min_value(&out[2u * i], mn);
			atomic_max_value(&out[2u * i + 1u], mx);
		}
	}
	if (g.counts != nullptr) {
		for (uint32_t i = threadIdx.x; i <= g.n_keys; i += 64u * WAVES) {
			const uint32_t c = s_cnt[i];
			if (c != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(g.counts) + i, static_cast<unsigned long long>(c)); }
		}
	}
	if (g.trace != nullptr && lane < 4u) { // the trace: one add per wavefront and counter
		const uint32_t mine = lane == 0u ? did[0] : lane == 1u ? did[1] : lane == 2u ? did[2] : did[3];
		if (mine != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(g.trace) + lane, static_cast<unsigned long long>(mine)); }
	}
}

// n_keys in 1 .. ALPGPU_KEYED_KEYS_MAX, the alignments checked by the caller: {+inf, -inf} and 0 everywhere
int launch_keyed_minmax_init(hipStream_t stream, void* d_out, uint64_t* d_counts, uint32_t n_keys, int value_bytes) {
	const dim3 grid((n_keys + 1u + 255u) / 256u);
	if (value_bytes == 8) {
		hipLaunchKernelGGL((k_keyed_minmax_init<double>), grid, dim3(256), 0, stream, static_cast<double*>(d_out), n_keys, d_counts);
	} else {
		hipLaunchKernelGGL((k_keyed_minmax_init<float>), grid, dim3(256), 0, stream, static_cast<float*>(d_out), n_keys, d_counts);
	}
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

// val->n_vectors == key->n_vectors in 1 .. 2^32 - 1, n_keys in 1 .. ALPGPU_KEYED_KEYS_MAX, the alignments checked by the caller.  The init and one
// launch of persistent workgroups.
int launch_keyed_minmax(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_keys, uint32_t n_keys,
                        void* d_out, uint64_t* d_counts, int value_bytes, int n_cus, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	KeyedMinmaxArgs args {};
	args.n_vectors = val->n_vectors;
	args.mask      = d_mask;
	args.keys      = d_keys;
	args.zones     = d_zones;
	args.out       = d_out;
	args.counts    = d_counts;
	args.trace     = d_trace;
	args.n_keys    = n_keys;
	const int rc = launch_keyed_minmax_init(stream, d_out, d_counts, n_keys, value_bytes);
	if (rc != ALPGPU_OK) { return rc; }
	const unsigned      grid = persistent_grid(val->n_vectors, kKmmWaves, n_cus, kKmmWgPerCu, 0, tuning != nullptr ? tuning->grid : 0u, kTuningGridMax);
	const ColumnStreams cv = column_streams(val), ck = column_streams(key);
	if (value_bytes == 8) {
		hipLaunchKernelGGL((k_keyed_minmax<8, kKmmWaves>), dim3(grid), dim3(kKmmThreads), 0, stream, cv, ck, args);
	} else {
		hipLaunchKernelGGL((k_keyed_minmax<4, kKmmWaves>), dim3(grid), dim3(kKmmThreads), 0, stream, cv, ck, args);
	}
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

} // namespace alpgpu
