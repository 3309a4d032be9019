// keyed_minmax_many_kernels.hip — keyed MIN / MAX for up to 2^20 keys (include/alpgpu.h, "keyed MIN / MAX, many keys": alpgpu_decode_keyed_minmax_many_*):
// the record {min, max} and the COUNT of a value column per key of a sorted key list, the key column decoded beside it, no decoded value reaching HBM.
// kmm_vector's per-vector flow (keyed_minmax_kernels.hip) on k_join_probe's list handling (join_kernels.hip, sorted_list.hpp): the keys no longer
// have to fit LDS, and the table is the call's outputs themselves.  The records' order key and the trace's classes are
// keyed_table.hpp's; the move was checked against the device assembly (profiles/r29_keyed_tables.txt).
//
//   k_keyed_minmax_many<VB, GLOBAL>
//                         persistent workgroups of kInWaves wavefronts.  The workgroup stages the sorted keys (GLOBAL: every stride-th of them, the
//                         pivots) into 32 KiB of static LDS, passes ONE workgroup barrier and then walks vectors v = wave id, wave id + waves, ...
//                         No wavefront meets another barrier, so the wavefronts of a workgroup need not make equal trips.
//   the keys              list_staging (persistent_launch.hpp) decides the tier: up to 4096 doubles / 8192 floats sit in LDS whole; a longer
//                         list leaves its pivots there and in_list_search finishes in the list's slice between two pivots, which L2 holds.
//   the table             d_out and d_counts, emptied by k_keyed_minmax_init (keyed_minmax_kernels.hip).  No LDS table, no flush, no scratch, no
//                         reduce kernel.
//   an update             a global integer atomic on the value's bits in the records' order (atomic_min_value / atomic_max_value of
//                         wave_minmax.hpp; agent scope; no compare-and-swap loop, no floating-point atomic).  A NaN value never reaches an atomic;
//                         it is counted only.
//   a step                64 values of both columns.  Lane l searches its key (in_list_search's lower bound, one ==).  m = the selected, matched lanes.
//                           all of m agree on one key     one wave_minmax (the other lanes fed minmax_skip), lane 0's guarded pair of atomics if
//                                                         the step had a number, one 64-bit count add of popcount(m);
//                           otherwise                     a lane reads its key's record from d_out with plain loads and issues an atomic only
//                                                         where its value improves on what it read, compared by the records' INTEGER order key
//                                                         (C's < would drop a -0.0 that arrives behind +0.0); one 64-bit add of 1 for the count.
//                         With d_counts == NULL no count atomic is issued at all.  kmany_update holds the guard and the argument for it.
//   zones                 kmm_vector's rules through sorted_list_zone: the key vector's record {min, max} (no NaNs) gives [j0, j1) = the keys it
//                         admits.  None: the selected bits are rows without a key, neither column is read.  min == max on a vector that is ALP
//                         without exceptions: every selected row has key j0; only the value vector is decoded, each lane keeps {mn, mx} over the 16
//                         steps in registers, then one wave_minmax and one guarded pair of atomics.  Otherwise the per-value search is over
//                         [j0, j1).  Every probe index is clamped.
//   rows without a key    summed per vector and added once, by lane 0.
//
// HBM traffic per vector: the bitmap's 128 bytes (none with a NULL bitmap) and, unless they or the zone record settle the vector, both vectors'
// descriptors, packed words and exception records; the keys (GLOBAL: the pivots) once per workgroup; GLOBAL, ceil(log2(stride)) probes of the list
// per value and the == fetch, from L2; per matched row a record read and, with counts, one atomic.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; launch bounds 512 = 2 wavefronts per SIMD and workgroup):
//   k_keyed_minmax_many<8, false>   124 VGPRs, 34816 B LDS, 4 waves per SIMD, no scratch (44 SGPRs kept in VGPR lanes)
//   k_keyed_minmax_many<8, true>    124 VGPRs, 34816 B LDS, 4 waves per SIMD, no scratch (52 SGPRs kept in VGPR lanes)
//   k_keyed_minmax_many<4, false>   99 VGPRs, 34816 B LDS, 4 waves per SIMD, no scratch (38 SGPRs kept in VGPR lanes)
//   k_keyed_minmax_many<4, true>    97 VGPRs, 34816 B LDS, 4 waves per SIMD, no scratch (47 SGPRs kept in VGPR lanes)
// amdgpu_waves_per_eu(4): left to itself the compiler takes 129 VGPRs for the double kernels (103 for float), one beyond the edge of 4 wavefronts
// per SIMD; asked for 4 it keeps 124 and still no scratch, so the search runs in batches of kStepBatch values in all four and no smaller batch
// was needed.  kManyWgPerCu = 2: two workgroups of 8 wavefronts are those 4 wavefronts per SIMD; their LDS, 2 x 34 KiB, decides nothing.
#include "keyed_table.hpp"

namespace alpgpu {

constexpr int kManyWgPerCu = 2;

struct KeyedManyArgs {
	uint64_t        n_vectors;
	const uint64_t* mask;   // nullable: every row
	void*           out;    // n_list records {min, max} of the columns' type, joined into
	uint64_t*       counts; // nullable: n_list + 1 words, added to
	uint64_t*       trace;  // nullable: 4 words, added to
};

// The number q (not a NaN) into record i of d_out, by the calling lane: the guard and the atomics.
// Why the guard is safe.  Between k_keyed_minmax_init and the kernel's end, out[2 i] only ever falls and out[2 i + 1] only ever rises in the records'
// order: every writer is an atomic minimum or maximum.  The plain loads below may be served by this CU's L1 or, for a record last written from another
// XCD, by a stale line of this XCD's L2; whatever they return is a value the word held at some time since the init kernel (the caches hold nothing
// older: the launch's acquire drops them), so it is no better than the word is now.  If q does not improve on the value read it does not improve on
// the word either, and leaving the atomic out changes nothing.  If q improves on a stale value but not on the word, the atomic is issued and changes
// nothing.  So a stale read causes a needless atomic and never a missed one.  Every improving value goes through an agent-scope atomic (atomicMin /
// atomicMax on global memory are device scope: they act on the one word, whichever XCD issues them); the records are final when the kernel ends.  The loaded value is never a NaN: the
// init kernel wrote an infinity and an atomic only ever carries a number.
template <class T>
__device__ __forceinline__ void kmany_update(T* out, uint32_t i, T q) {
	const auto k = order_key(q);
	if (k < order_key(out[2u * i])) { atomic_min_value(&out[2u * i], q); }
	if (k > order_key(out[2u * i + 1u])) { atomic_max_value(&out[2u * i + 1u], q); }
}

// a wave-uniform record {mn, mx} (lane 0 acts) into record i, unless it is the empty one.  mn and mx go through the same guard: a sorted key column
// sends every step here with the same i, and once the record holds the key's range its steps cost two loads and no atomic.
template <class T>
__device__ __forceinline__ void kmany_join(T* out, uint32_t i, T mn, T mx, uint32_t lane) {
	if (lane == 0u && mn <= mx) { // ({+inf, -inf}: no number was fed; -0.0 <= +0.0 and inf <= inf hold)
		if (order_key(mn) < order_key(out[2u * i])) { atomic_min_value(&out[2u * i], mn); }
		if (order_key(mx) > order_key(out[2u * i + 1u])) { atomic_max_value(&out[2u * i + 1u], mx); }
	}
}

__device__ __forceinline__ void kmany_count(uint64_t* counts, uint32_t i, uint32_t n) {
	atomicAdd(reinterpret_cast<unsigned long long*>(counts) + i, static_cast<unsigned long long>(n));
}

// One step's selected, matched lanes m (wave-uniform) into the call's table: lane l holds the canonical value q and the key index idx (< n_list always).
template <class T>
__device__ __forceinline__ void kmany_step(T* out, uint64_t* counts, uint64_t m, uint32_t idx, T q, uint32_t lane) {
	if (m == 0ull) { return; }
	const bool     in    = (m >> lane) & 1ull;
	const uint32_t first = static_cast<uint32_t>(__builtin_amdgcn_readlane(idx, static_cast<uint32_t>(__builtin_ctzll(m))));
	if ((m & ballot64(idx == first)) == m) { // the step's lanes agree on one key
		T mn = pos_inf<T>(), mx = -pos_inf<T>();
		minmax_feed(mn, mx, in ? q : minmax_skip<T>()); // (a NaN q is a quiet one: skipped)
		wave_minmax<T>(mn, mx);
		kmany_join(out, first, mn, mx, lane);
		if (counts != nullptr && lane == 0u) { kmany_count(counts, first, static_cast<uint32_t>(__builtin_popcountll(m))); }
		return;
	}
	if (in) {
		if (q == q) { kmany_update(out, idx, q); }
		if (counts != nullptr) { kmany_count(counts, idx, 1u); }
	}
}

// One vector pair by one wavefront.  Returns the class of the trace it fell into.  counts[n_list] takes the selected rows without a key.
template <int VB, bool GLOBAL>
__device__ __forceinline__ uint32_t kmany_vector(const ColumnStreams& cv, const ColumnStreams& ck, const InArgs& g, const KeyedManyArgs& a, uint64_t v, uint32_t wave, uint32_t lane,
                                                 const typename DecodeVec<VB>::T* s_list, uint64_t (&s_exc)[kInWaves][2][16]) {
	typedef typename DecodeVec<VB>::T T;
	const T*       list     = static_cast<const T*>(g.list);
	T*             out      = static_cast<T*>(a.out);
	const bool     counted  = a.counts != nullptr;
	const uint32_t last_key = g.n_list - 1u;
	// 1. the selected bits, lane m < 16 holding word m
	uint64_t sel;
	if (!selected_words(a.mask, 0ull, a.n_vectors << 10, v, lane, sel)) { return kVectorSkipZero; }

	// 2. the part [j0, j1) of the keys that the key vector's zone record admits: all of them without a record or with a NaN bound
	uint32_t j0 = 0u, j1 = g.n_list;
	if (g.zones != nullptr) {
		sorted_list_zone<VB, GLOBAL>(s_list, list, g, v, j0, j1); // the first key >= min, the first key > max
		if (j1 <= j0) { // no key lies in the record: rows without a key
			if (counted) {
				const uint32_t n = selected_count(sel);
				if (lane == 63u) { kmany_count(a.counts, g.n_list, n); }
			}
			return kVectorNoEntry;
		}
		const T* zone = static_cast<const T*>(g.zones) + 2 * v; // (wave-uniform)
		if (zone[0] == zone[1] && alp_without_exceptions(ck.descs[v])) { // (no NaN bound is equal) no NaN can hide here: every selected row has key j0; the value vector alone is decoded
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
			const uint32_t i0 = j0 < last_key ? j0 : last_key; // (j0 < j1 <= n_list: the clamp changes nothing and costs one instruction)
			kmany_join(out, i0, mn, mx, lane);
			if (counted && lane == 0u) { kmany_count(a.counts, i0, n_rows); }
			return kVectorOneEntry;
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
		// 5. the batch's keys, searched together: the lower bound and one ==.  A NaN key is never equal; the index read is clamped to the list.
		uint32_t at[kStepBatch];
		in_list_search<VB, GLOBAL, kStepBatch>(s_list, list, g, j0, j1, k, 0u, at);
		T e[kStepBatch];
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) { e[i] = sorted_list_at<VB, GLOBAL>(s_list, list, g, at[i]); }
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			const uint32_t idx = at[i] < last_key ? at[i] : last_key; // the element sorted_list_at read
			const uint64_t w   = readlane64(sel, b + i);
			const uint64_t m   = w & ballot64(e[i] == k[i]);
			unmatched += static_cast<uint32_t>(__builtin_popcountll(w & ~m));
			kmany_step<T>(out, a.counts, m, idx, q[i], lane);
		}
	}
	if (counted && unmatched != 0u && lane == 0u) { kmany_count(a.counts, g.n_list, unmatched); }
	return kVectorDecoded;
}

template <int VB, bool GLOBAL>
__global__ __launch_bounds__(kInThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_keyed_minmax_many(const ColumnStreams cv, const ColumnStreams ck, const InArgs g, const KeyedManyArgs a) {
	typedef typename DecodeVec<VB>::T T;
	__shared__ T        s_list[kInLdsBytes / VB];
	__shared__ uint64_t s_exc[kInWaves][2][16]; // per wavefront and column: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;

	// 0. the keys (GLOBAL: their pivots) into LDS, once per workgroup; the one workgroup barrier of the kernel
	sorted_list_stage<VB, GLOBAL>(s_list, static_cast<const T*>(g.list), g);
	__syncthreads();

	const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * kInWaves;
	uint32_t       did[4]  = {0u, 0u, 0u, 0u};
	for (uint64_t v = static_cast<uint64_t>(blockIdx.x) * kInWaves + wave; v < a.n_vectors; v += n_waves) {
		const uint32_t what = kmany_vector<VB, GLOBAL>(cv, ck, g, a, v, wave, lane, s_list, s_exc);
#pragma unroll
		for (uint32_t i = 0; i < 4u; ++i) { did[i] += what == i ? 1u : 0u; }
	}
	if (a.trace != nullptr && lane < 4u) { // the trace: one add per wavefront and counter
		const uint32_t mine = lane == 0u ? did[0] : lane == 1u ? did[1] : lane == 2u ? did[2] : did[3];
		if (mine != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(a.trace) + lane, static_cast<unsigned long long>(mine)); }
	}
}

template <int VB>
static int launch_many_vb(hipStream_t stream, const ColumnStreams& cv, const ColumnStreams& ck, const InArgs& g, const KeyedManyArgs& a, unsigned grid) {
	if (g.stride > 1u) {
		hipLaunchKernelGGL((k_keyed_minmax_many<VB, true>), dim3(grid), dim3(kInThreads), 0, stream, cv, ck, g, a);
	} else {
		hipLaunchKernelGGL((k_keyed_minmax_many<VB, false>), dim3(grid), dim3(kInThreads), 0, stream, cv, ck, g, a);
	}
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

// val->n_vectors == key->n_vectors in 1 .. 2^32 - 1, n_keys in 1 .. ALPGPU_KEYED_MANY_KEYS_MAX, the alignments checked by the caller.  The init
// kernel of keyed_minmax_kernels.hip and one launch of persistent workgroups.
int launch_keyed_minmax_many(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_keys,
                             uint32_t n_keys, void* d_out, uint64_t* d_counts, int value_bytes, int n_cus, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	const int rc = launch_keyed_minmax_init(stream, d_out, d_counts, n_keys, value_bytes);
	if (rc != ALPGPU_OK) { return rc; }
	KeyedManyArgs a {};
	a.n_vectors = val->n_vectors;
	a.mask      = d_mask;
	a.out       = d_out;
	a.counts    = d_counts;
	a.trace     = d_trace;
	const ListStaging staging = list_staging(n_keys, value_bytes);
	InArgs            g {};
	g.list   = d_keys;
	g.zones  = d_zones;
	g.n_list = n_keys;
	g.stride = staging.stride;
	g.n_piv  = staging.n_piv;
	const unsigned      grid = persistent_grid(val->n_vectors, kInWaves, n_cus, kManyWgPerCu, 0, tuning != nullptr ? tuning->grid : 0u, kTuningGridMax);
	const ColumnStreams cv = column_streams(val), ck = column_streams(key);
	return value_bytes == 8 ? launch_many_vb<8>(stream, cv, ck, g, a, grid) : launch_many_vb<4>(stream, cv, ck, g, a, grid);
}

} // namespace alpgpu
