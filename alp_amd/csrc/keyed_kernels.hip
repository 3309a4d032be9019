// keyed_kernels.hip — keyed aggregation (include/alpgpu.h, "keyed aggregation": alpgpu_decode_keyed_sum_*): SUM and COUNT of a value column per key of a
// sorted key list, the key column decoded beside it, no decoded value reaching HBM.  The parts are k_pair's side-by-side decode (register_decode.hpp),
// lds_bound over the staged keys (sorted_list.hpp) and selected_words with the constant-vector predicate (persistent_scan.hpp).  The step (keyed_step)
// and the tiers are keyed_table.hpp's, shared with bucket_kernels.hip; the move was checked against the device assembly (profiles/r29_keyed_tables.txt).
//
//   k_keyed_init          zeroes the counts and the scratch's header (the stripe ticket): a kernel, no memset node (mask_kernels.hip says why).
//   k_keyed_sum<VB, KCAP, WAVES>
//                         persistent workgroups of WAVES wavefronts.  The workgroup stages the keys into LDS and passes ONE barrier; from there on its
//                         wavefronts share nothing and wait for nobody.  A wavefront takes a stripe s (the vectors [s L, min((s + 1) L, n_vectors)))
//                         by an integer ticket, zeroes its PRIVATE table of n_keys doubles and n_keys 32-bit counts in LDS, walks the stripe's
//                         vectors in ascending order, stores its n_keys partials into row s of the scratch with plain vector stores and adds its
//                         counts into d_counts by integer atomics.  Which wavefront takes which stripe does not enter a stripe's partials.
//   a step                64 values of both columns.  Lane l searches its key (lds_bound's lower bound, one ==).  m = the selected, matched lanes.
//                           all of m agree on one key     one wave_tree_sum_f64 (+0.0 in the other lanes), one LDS read-modify-write by lane 0;
//                           otherwise                     every lane of m adds 1 to its key's count by an LDS integer atomic and reads the count
//                                                         before and behind: a lane that saw it grow by exactly 1 is alone with its key in this
//                                                         step and adds its own value to the key's sum (the tree of one value and 63 times +0.0 is
//                                                         that value, or +0.0 for -0.0, and adding either to an accumulator that began at +0.0
//                                                         gives the same bits: DESIGN.md, "Keyed aggregation"); the lanes left go key by key
//                                                         through ballot, tree and lane 0's read-modify-write, in the order of their first lanes.
//                         Two keys' accumulators never meet, so the order among keys within a step is free; one key's adds are in (v, m) order.
//   zones                 the key vector's record {min, max} (no NaNs) is searched by the whole wavefront: [j0, j1) = the keys it admits.  None: the
//                         selected bits are rows without a key, neither column is read.  min == max on a vector that is ALP without exceptions: every
//                         selected row has key j0, the key vector's packed words are not requested and only the value vector is decoded.  Otherwise
//                         the per-value search is over [j0, j1).  Every probe index is clamped to the keys staged.
//   k_keyed_reduce        one workgroup per key: the S partials of the key's column of the scratch by k_tree_sum's levels (blocks of 1024 padded with
//                         +0.0: (e0 + e1) + (e2 + e3), the wave tree, (s0 + s1) + (s2 + s3)), at most two levels for S <= 4096.
//
// LDS banks: a wavefront's sums are n_keys consecutive doubles and its counts n_keys consecutive words, so the 64 lanes of a step with dense,
// distinct keys read and write 64 neighbouring doubles (ds_read_b64: 64 banks) and do not meet on one bank; only equal keys meet, and those are
// either the one-key step (one lane) or the atomic's own serialisation.
//
// HBM traffic per vector: the bitmap's 128 bytes (none with a NULL bitmap) and, unless they or the zone record settle the vector, both vectors'
// descriptors, packed words and exception records; 8 n_keys bytes per stripe into the scratch; the keys once per workgroup.
//
// Two capacity tiers, so that a call with few keys is not held to the occupancy of 1024: KCAP = 256 with 8 wavefronts (two workgroups per CU, what
// the registers admit under 4 waves per SIMD), KCAP = 1024 with 12 wavefronts (one workgroup per CU, what the LDS admits).
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; launch bounds 512 and 768):
//   k_keyed_sum<8,  256,  8>   126 VGPRs,  28672 B LDS, 4 waves per SIMD, no scratch (53 SGPRs kept in VGPR lanes)
//   k_keyed_sum<8, 1024, 12>   125 VGPRs, 158720 B LDS, 3 waves per SIMD, no scratch (50 SGPRs kept in VGPR lanes)
//   (the small tier sits 2 registers under the 128 that 4 waves per SIMD, two workgroups per CU, allow: a change here is checked against that)
//   (VB = 4, the float kernels, are templates here and NOT instantiated: the call is built for double columns only)
//   k_keyed_reduce              15 VGPRs,     64 B LDS, 8 waves per SIMD, no scratch;  k_keyed_init  6 VGPRs, no LDS, no scratch
// The lone-lane shortcut of a step was measured against the step without it (-DALPGPU_KEYED_BASELINE_STEP, tools/time_keyed.py --ab;
// profiles/r25_keyed_sum.txt, second part; DESIGN.md, "Keyed aggregation").
#include "keyed_table.hpp"

namespace alpgpu {

struct KeyedArgs {
	uint64_t        n_vectors;
	uint64_t        stripe_vectors; // L
	uint32_t        n_stripes;      // S = ceil(n_vectors / L) <= ALPGPU_KEYED_STRIPES_MAX
	uint32_t        n_keys;         // 1 .. ALPGPU_KEYED_KEYS_MAX
	const uint64_t* mask;           // nullable: every row
	const void*     keys;           // n_keys sorted elements of the key column's type
	const void*     zones;          // nullable: one record {min, max} per key vector
	uint32_t*       ticket;         // the scratch's header: the next stripe
	double*         partials;       // [S][n_keys]
	uint64_t*       counts;         // nullable: n_keys + 1 words, added to
	uint64_t*       trace;          // nullable: 4 words, added to
};

// One vector pair by one wavefront.  Returns the class of the trace it fell into; unmatched (wave-uniform) takes the selected rows without a key.
template <int VB, int WAVES>
__device__ __forceinline__ uint32_t keyed_vector(const ColumnStreams& cv, const ColumnStreams& ck, const KeyedArgs& g, uint64_t v, uint32_t wave, uint32_t lane,
                                                 const typename DecodeVec<VB>::T* s_keys, double* s_sums, uint32_t* s_cnt, uint64_t (&s_exc)[WAVES][2][16], uint32_t& unmatched) {
	typedef typename DecodeVec<VB>::T T;
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
				unmatched += __builtin_amdgcn_readlane(selected_count(sel), 63);
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
				double   acc = 0.0; // lane 0's: the key's accumulator, read once and written once (no other key is touched in between)
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
		// 5. the batch's keys, searched together: the lower bound and one ==.  A NaN key is never equal; the index read is clamped to the keys staged.
		uint32_t at[kStepBatch];
		lds_bound<T, kStepBatch>(s_keys, last_key, j0, j1, k, 0u, at);
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			const uint32_t idx  = at[i] < last_key ? at[i] : last_key;
			const uint64_t w    = readlane64(sel, b + i);
			const uint64_t m    = w & ballot64(s_keys[idx] == k[i]);
			unmatched += static_cast<uint32_t>(__builtin_popcountll(w & ~m));
			keyed_step(s_sums, s_cnt, m, idx, x[i], lane);
		}
	}
	return kVectorDecoded;
}

__global__ __launch_bounds__(256) void k_keyed_init(uint64_t* counts, uint32_t n_counts, uint64_t* header) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (counts != nullptr && i < n_counts) { counts[i] = 0ull; }
	if (i < 8u) { header[i] = 0ull; }
}

template <int VB, uint32_t KCAP, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_keyed_sum(const ColumnStreams cv, const ColumnStreams ck, const KeyedArgs g) {
	typedef typename DecodeVec<VB>::T T;
	__shared__ double   s_sums[WAVES][KCAP]; // per wavefront: the stripe's partials
	__shared__ uint32_t s_cnt[WAVES][KCAP];  // ... and counts
	__shared__ T        s_keys[KCAP];
	__shared__ uint64_t s_exc[WAVES][2][16]; // per wavefront and column: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;

	// 0. the keys into LDS, once per workgroup; the one barrier
	const T* keys = static_cast<const T*>(g.keys);
	for (uint32_t i = threadIdx.x; i < g.n_keys; i += 64u * WAVES) { s_keys[i] = keys[i]; }
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
		for (uint32_t i = lane; i < g.n_keys; i += 64u) {
			sums[i] = 0.0;
			cnt[i]  = 0u;
		}
		wave_lds_sync();
		// 3. the stripe's vectors, ascending
		const uint64_t v0 = static_cast<uint64_t>(s) * g.stripe_vectors;
		const uint64_t v1 = v0 + g.stripe_vectors < g.n_vectors ? v0 + g.stripe_vectors : g.n_vectors;
		uint32_t       unmatched = 0u;
		for (uint64_t v = v0; v < v1; ++v) {
			const uint32_t what = keyed_vector<VB, WAVES>(cv, ck, g, v, wave, lane, s_keys, sums, cnt, s_exc, unmatched);
#pragma unroll
			for (uint32_t i = 0; i < 4u; ++i) { did[i] += what == i ? 1u : 0u; }
		}
		wave_lds_sync();
		// 4. the partials into row s of the scratch, 5. the counts into the call's
		double* row = g.partials + static_cast<uint64_t>(s) * g.n_keys;
		for (uint32_t i = lane; i < g.n_keys; i += 64u) {
			row[i] = sums[i];
			if (g.counts != nullptr) {
				const uint32_t n = cnt[i];
				if (n != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(g.counts) + i, static_cast<unsigned long long>(n)); }
			}
		}
		if (g.counts != nullptr && unmatched != 0u && lane == 0u) {
			atomicAdd(reinterpret_cast<unsigned long long*>(g.counts) + g.n_keys, static_cast<unsigned long long>(unmatched));
		}
		wave_lds_sync();
	}
	if (g.trace != nullptr && lane < 4u) { // the trace: one add per wavefront and counter
		const uint32_t mine = lane == 0u ? did[0] : lane == 1u ? did[1] : lane == 2u ? did[2] : did[3];
		if (mine != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(g.trace) + lane, static_cast<unsigned long long>(mine)); }
	}
}

// out[key] = k_tree_sum's tree over partials[0 .. n_stripes)[key]; one workgroup per key, n_stripes in 1 .. ALPGPU_KEYED_STRIPES_MAX
__global__ __launch_bounds__(256) void k_keyed_reduce(const double* __restrict__ partials, uint32_t n_stripes, uint32_t n_keys, double* __restrict__ out) {
	__shared__ double s_w[4];
	__shared__ double s_b[4];
	const uint32_t key    = blockIdx.x;
	const uint32_t blocks = (n_stripes + 1023u) / 1024u; // <= 4
	for (uint32_t b = 0; b < blocks; ++b) {
		const uint32_t i0 = 1024u * b + 4u * threadIdx.x;
		double         e[4];
#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) { e[j] = i0 + j < n_stripes ? partials[static_cast<uint64_t>(i0 + j) * n_keys + key] : 0.0; }
		const double w = wave_tree_sum_f64((e[0] + e[1]) + (e[2] + e[3]));
		if ((threadIdx.x & 63u) == 0u) { s_w[threadIdx.x >> 6] = w; }
		__syncthreads();
		if (threadIdx.x == 0u) { s_b[b] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]); }
		__syncthreads();
	}
	if (blocks == 1u) {
		if (threadIdx.x == 0u) { out[key] = s_b[0]; }
		return;
	}
	double e[4]; // the second level: the blocks' sums as one block of 1024 padded with +0.0
#pragma unroll
	for (uint32_t j = 0; j < 4u; ++j) { e[j] = 4u * threadIdx.x + j < blocks ? s_b[(4u * threadIdx.x + j) & 3u] : 0.0; }
	const double w = wave_tree_sum_f64((e[0] + e[1]) + (e[2] + e[3]));
	if ((threadIdx.x & 63u) == 0u) { s_w[threadIdx.x >> 6] = w; }
	__syncthreads();
	if (threadIdx.x == 0u) { out[key] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]); }
}

template <int VB>
static void keyed_launch(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const KeyedArgs& args, int n_cus, uint32_t grid_override) {
	const ColumnStreams cv = column_streams(val), ck = column_streams(key);
	if (args.n_keys <= kKeyedSmallKeys) {
		const unsigned grid = persistent_grid(args.n_stripes, kKeyedSmallWaves, n_cus, kKeyedSmallWgPerCu, 0, grid_override, kTuningGridMax);
		hipLaunchKernelGGL((k_keyed_sum<VB, kKeyedSmallKeys, kKeyedSmallWaves>), dim3(grid), dim3(64 * kKeyedSmallWaves), 0, stream, cv, ck, args);
	} else {
		const unsigned grid = persistent_grid(args.n_stripes, kKeyedLargeWaves, n_cus, kKeyedLargeWgPerCu, 0, grid_override, kTuningGridMax);
		hipLaunchKernelGGL((k_keyed_sum<VB, ALPGPU_KEYED_KEYS_MAX, kKeyedLargeWaves>), dim3(grid), dim3(64 * kKeyedLargeWaves), 0, stream, cv, ck, args);
	}
}

// val->n_vectors == key->n_vectors in 1 .. 2^32 - 1, n_keys in 1 .. ALPGPU_KEYED_KEYS_MAX, the alignments checked by the caller; d_scratch: 64 bytes of
// header and keyed_stripes(n_vectors) rows of n_keys doubles.  The init, one launch of persistent workgroups, the reduce.
int launch_keyed_sum(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_keys, uint32_t n_keys,
                     double* d_sums, uint64_t* d_counts, void* d_scratch, int value_bytes, int n_cus, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	KeyedArgs args {};
	args.n_vectors      = val->n_vectors;
	args.stripe_vectors = keyed_stripe_vectors(val->n_vectors);
	args.n_stripes      = static_cast<uint32_t>(keyed_stripes(val->n_vectors));
	args.n_keys         = n_keys;
	args.mask           = d_mask;
	args.keys           = d_keys;
	args.zones          = d_zones;
	args.ticket         = static_cast<uint32_t*>(d_scratch);
	args.partials       = reinterpret_cast<double*>(static_cast<uint8_t*>(d_scratch) + 64);
	args.counts         = d_counts;
	args.trace          = d_trace;
	hipLaunchKernelGGL(k_keyed_init, dim3((n_keys + 1u + 255u) / 256u), dim3(256), 0, stream, d_counts, n_keys + 1u, static_cast<uint64_t*>(d_scratch));
	if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	const uint32_t grid_override = tuning != nullptr ? tuning->grid : 0u;
	if (value_bytes != 8) { return ALPGPU_ERR_INVALID; } // (double columns only: the float kernels are not built, include/alpgpu.h says why)
	keyed_launch<8>(stream, val, key, args, n_cus, grid_override);
	if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	hipLaunchKernelGGL(k_keyed_reduce, dim3(n_keys), dim3(256), 0, stream, args.partials, args.n_stripes, n_keys, d_sums);
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

} // namespace alpgpu
