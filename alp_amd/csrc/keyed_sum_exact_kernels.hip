// keyed_sum_exact_kernels.hip — the exact keyed SUM for up to 2^20 keys (include/alpgpu.h, "exact keyed SUM": alpgpu_decode_keyed_exact_sum_*): per key
// of a sorted key list the correctly rounded real sum and the COUNT of a value column, the key column decoded beside it, no decoded value reaching HBM.
// k_keyed_minmax_many's skeleton (keyed_minmax_many_kernels.hip: persistent wavefronts, sorted_list.hpp's staging and pivot tier, register_decode.hpp's
// side-by-side decode, the zone rules) with another update: every value is added as an integer to its key's fixed-point entry (exact_sum.hpp: 66 limbs
// of int64 and a word of flags per key, in the caller's table in device memory), and a second kernel rounds every entry once.  Integer adds are
// associative, so neither the grid nor the order in which rows arrive enters a limb: the sums are a function of the inputs alone.
//
//   k_keyed_exact_zero              the table and the counts zeroed (not with accumulate); not a memset node ("Histograms").
//   k_keyed_sum_exact<VB, GLOBAL>   persistent workgroups of kInWaves wavefronts; the keys (GLOBAL: their pivots) staged into 32 KiB of LDS, ONE workgroup
//                                   barrier, then vectors v = wave id, wave id + waves, ...  No floating-point atomic, no compare-and-swap loop, no
//                                   workgroup waits for another.
//   a step                          64 values of both columns; lane l searches its key (the lower bound and one ==).  m = the selected, matched lanes.
//                                   A NaN or infinite value ORs its flag into its key's flags word (an integer atomic; the rare path) and adds nothing.
//     m agrees on one key and the lanes' first limbs span at most 3   (values within 2^64 of each other do): each lane places its three chunks in a
//                                   frame of 5 limbs from the lowest first limb on, the frame is summed over the wavefront by integer adds (DPP; any tree
//                                   is exact) and lane 63 issues at most 5 atomics, and one for the count.  A sorted or clustered key column takes this
//                                   arm almost everywhere; a constant-key vector (the zone shortcut) is 16 such steps.
//     any other step                each lane issues its up-to-three 64-bit integer atomic adds without return, and its count atomic (one lane for all
//                                   where the step agrees on its key) unless d_counts == NULL.
//   k_keyed_sum_exact_finish        one thread per key: exact_round_limbs_bits of its entry into d_sums.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; launch bounds 512 = 2 wavefronts per SIMD and workgroup): see
// DESIGN.md, "Exact keyed SUM"; no kernel of this file uses scratch memory.
#include "exact_sum.hpp"
#include "keyed_table.hpp"

namespace alpgpu {

constexpr int      kExactWgPerCu = 2;
constexpr uint32_t kExactBatch   = 2; // steps of a vector requested and searched together (kStepBatch = 4 leaves k_keyed_sum_exact<8, true> 12 bytes of scratch)

struct KeyedExactArgs {
	uint64_t        n_vectors;
	const uint64_t* mask;   // nullable: every row
	int64_t*        table;  // n_list entries of kExactKeyWords words, added to
	uint64_t*       counts; // nullable: n_list + 1 words, added to
	uint64_t*       trace;  // nullable: 6 words, added to
};

constexpr uint32_t kStepNone = 0u, kStepInRegisters = 1u, kStepByLane = 2u; // what a step did: the trace's words 4 and 5 count the last two

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t dpp_take_u32(uint32_t old, uint32_t v) {
	return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(static_cast<int>(old), static_cast<int>(v), CTRL, ROW_MASK, 0xf, false));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int64_t dpp_take_i64(int64_t v) { // 0 where the pattern has no source lane
	const uint64_t b = static_cast<uint64_t>(v);
	const uint32_t lo = dpp_take_u32<CTRL, ROW_MASK>(0u, static_cast<uint32_t>(b)), hi = dpp_take_u32<CTRL, ROW_MASK>(0u, static_cast<uint32_t>(b >> 32));
	return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}
// the sum of the 64 lanes' values in lane 63 (wave_tree_sum_f64's tree, on integers: exact whatever the tree)
__device__ __forceinline__ int64_t wave_sum_i64_lane63(int64_t v) {
	v += dpp_take_i64<0x111, 0xf>(v); // row_shr:1
	v += dpp_take_i64<0x112, 0xf>(v); // row_shr:2
	v += dpp_take_i64<0x114, 0xf>(v); // row_shr:4
	v += dpp_take_i64<0x118, 0xf>(v); // row_shr:8
	v += dpp_take_i64<0x142, 0xa>(v); // row_bcast:15 into rows 1 and 3
	v += dpp_take_i64<0x143, 0xc>(v); // row_bcast:31 into rows 2 and 3
	return v;
}
// the minimum of the lanes' mn and the maximum of their mx, wave-uniform
__device__ __forceinline__ void wave_min_max_u32(uint32_t& mn, uint32_t& mx) {
#define ALPGPU_EXACT_LEVEL(CTRL, ROW_MASK)                                                                              \
	{                                                                                                                   \
		const uint32_t a = dpp_take_u32<CTRL, ROW_MASK>(~0u, mn), b = dpp_take_u32<CTRL, ROW_MASK>(0u, mx);             \
		mn = a < mn ? a : mn, mx = b > mx ? b : mx;                                                                     \
	}
	ALPGPU_EXACT_LEVEL(0x111, 0xf)
	ALPGPU_EXACT_LEVEL(0x112, 0xf)
	ALPGPU_EXACT_LEVEL(0x114, 0xf)
	ALPGPU_EXACT_LEVEL(0x118, 0xf)
	ALPGPU_EXACT_LEVEL(0x142, 0xa)
	ALPGPU_EXACT_LEVEL(0x143, 0xc)
#undef ALPGPU_EXACT_LEVEL
	mn = __builtin_amdgcn_readlane(mn, 63);
	mx = __builtin_amdgcn_readlane(mx, 63);
}

__device__ __forceinline__ void kexact_add(int64_t* word, int64_t v) { // (no return value is used: an atomic without return)
	atomicAdd(reinterpret_cast<unsigned long long*>(word), static_cast<unsigned long long>(v));
}
__device__ __forceinline__ void kexact_count(uint64_t* counts, uint32_t i, uint32_t n) {
	atomicAdd(reinterpret_cast<unsigned long long*>(counts) + i, static_cast<unsigned long long>(n));
}

// One step's selected, matched lanes m (wave-uniform) into the call's table: lane l holds the value x (widened, exactly) and the key index idx
// (< n_list always).  Returns what the step did (wave-uniform).
__device__ __forceinline__ uint32_t kexact_step(int64_t* table, uint64_t* counts, uint64_t m, uint32_t idx, double x, uint32_t lane) {
	if (m == 0ull) { return kStepNone; }
	const bool       in    = (m >> lane) & 1ull;
	const ExactSplit s     = exact_split(static_cast<uint64_t>(__double_as_longlong(x)));
	const uint32_t   first = static_cast<uint32_t>(__builtin_amdgcn_readlane(idx, static_cast<uint32_t>(__builtin_ctzll(m))));
	const bool       agree = (m & ballot64(idx == first)) == m; // the step's lanes agree on one key
	int64_t*         mine  = table + static_cast<uint64_t>(idx) * kExactKeyWords; // this lane's entry (idx < n_list in every lane)
	if ((m & ballot64(s.flags != 0u)) != 0ull) { // the rare path: a NaN or an infinity among the step's values
		if (in && s.flags != 0u) { atomicOr(reinterpret_cast<unsigned long long*>(mine + kExactLimbs), static_cast<unsigned long long>(s.flags)); }
	}
	const bool live = in && (s.chunk[0] | s.chunk[1] | s.chunk[2]) != 0u; // (a flagged value and a zero have no chunk)
	int64_t    c[3];
#pragma unroll
	for (uint32_t k = 0; k < 3u; ++k) { c[k] = !live ? 0 : s.negative ? -static_cast<int64_t>(s.chunk[k]) : static_cast<int64_t>(s.chunk[k]); }
	if (agree) {
		if (counts != nullptr && lane == 63u) { kexact_count(counts, first, static_cast<uint32_t>(__builtin_popcountll(m))); }
		uint32_t lo = live ? s.limb : ~0u, hi = live ? s.limb : 0u;
		wave_min_max_u32(lo, hi);
		if (lo == ~0u) { return kStepInRegisters; } // zeros and flagged values only: nothing to add
		if (hi - lo <= 2u) {                        // every live lane's chunks lie in the limbs lo .. lo + 4
			const uint32_t d = s.limb - lo;         // 0 .. 2 in a live lane; a lane that is not live holds zeros
			int64_t        f[5];
			f[0] = d == 0u ? c[0] : 0;
			f[1] = d == 0u ? c[1] : d == 1u ? c[0] : 0;
			f[2] = d == 0u ? c[2] : d == 1u ? c[1] : c[0];
			f[3] = d == 1u ? c[2] : d == 2u ? c[1] : 0;
			f[4] = d == 2u ? c[2] : 0;
			int64_t* entry = table + static_cast<uint64_t>(first) * kExactKeyWords + lo;
#pragma unroll
			for (uint32_t k = 0; k < 5u; ++k) {
				if (ballot64(f[k] != 0) != 0ull) { // (wave-uniform: a frame limb no lane reaches costs one compare)
					const int64_t t = wave_sum_i64_lane63(f[k]);
					if (lane == 63u && t != 0 && lo + k < kExactLimbs) { kexact_add(entry + k, t); } // (a non-zero limb of the frame is at most hi + 2 <= 65)
				}
			}
			return kStepInRegisters;
		}
	} else if (counts != nullptr && in) {
		kexact_count(counts, idx, 1u);
	}
	if (live) {
#pragma unroll
		for (uint32_t k = 0; k < 3u; ++k) {
			if (c[k] != 0) { kexact_add(mine + s.limb + k, c[k]); } // (limb <= 63: the highest is 65)
		}
	}
	return kStepByLane;
}

// One vector pair by one wavefront.  Returns the class of the trace it fell into; steps[1], steps[2] take the steps by what they did.
template <int VB, bool GLOBAL>
__device__ __forceinline__ uint32_t kexact_vector(const ColumnStreams& cv, const ColumnStreams& ck, const InArgs& g, const KeyedExactArgs& a, uint64_t v, uint32_t wave, uint32_t lane,
                                                  const typename DecodeVec<VB>::T* s_list, uint64_t (&s_exc)[kInWaves][2][16], uint32_t (&steps)[3]) {
	typedef typename DecodeVec<VB>::T T;
	const T*       list     = static_cast<const T*>(g.list);
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
				if (lane == 63u) { kexact_count(a.counts, g.n_list, n); }
			}
			return kVectorNoEntry;
		}
		const T* zone = static_cast<const T*>(g.zones) + 2 * v; // (wave-uniform)
		if (zone[0] == zone[1] && alp_without_exceptions(ck.descs[v])) { // (no NaN bound is equal) every selected row has key j0; the value vector alone is decoded
			const DecodeVec<VB> A = decode_vec_load<VB>(cv, v);
			if (A.cnt > 0) {
				if (lane < 16u) { s_exc[wave][0][lane] = 0ull; }
				wave_lds_sync();
				mark_exceptions<VB>(A, s_exc[wave][0], lane);
				wave_lds_sync();
			}
			uint32_t       exc_a = 0;
			const uint32_t i0    = j0 < last_key ? j0 : last_key; // (j0 < j1 <= n_list: the clamp changes nothing and costs one instruction)
			for (uint32_t b = 0; b < 16u; b += kExactBatch) {
				StepBatch<VB, kExactBatch> Ra;
				step_request(A, s_exc[wave][0], b, lane, exc_a, Ra);
#pragma unroll
				for (uint32_t i = 0; i < kExactBatch; ++i) {
					const double   x    = static_cast<double>(step_value(A, Ra, b, i, lane));
					const uint32_t what = kexact_step(a.table, a.counts, readlane64(sel, b + i), i0, x, lane);
#pragma unroll
					for (uint32_t w = 1; w < 3u; ++w) { steps[w] += what == w ? 1u : 0u; }
				}
			}
			return kVectorOneEntry;
		}
	}

	// 3. both descriptors and dictionaries, both exception masks
	const DecodeVec<VB> A = decode_vec_load<VB>(cv, v);
	const DecodeVec<VB> B = decode_vec_load<VB>(ck, v);
	exception_masks(A, B, s_exc, wave, lane);

	uint32_t exc_a = 0, exc_b = 0; // exceptions of the steps done
	uint32_t unmatched = 0u;       // wave-uniform
	for (uint32_t b = 0; b < 16u; b += kExactBatch) {
		// 4. every load of kExactBatch steps of BOTH vectors is requested before the first is used
		StepBatch<VB, kExactBatch> Ra, Rb;
		step_request(A, s_exc[wave][0], b, lane, exc_a, Ra);
		step_request(B, s_exc[wave][1], b, lane, exc_b, Rb);
		T q[kExactBatch], k[kExactBatch];
#pragma unroll
		for (uint32_t i = 0; i < kExactBatch; ++i) {
			q[i] = step_value(A, Ra, b, i, lane);
			k[i] = step_value(B, Rb, b, i, lane);
		}
		// 5. the batch's keys, searched together: the lower bound and one ==.  A NaN key is never equal; the index read is clamped to the list.
		uint32_t at[kExactBatch];
		in_list_search<VB, GLOBAL, kExactBatch>(s_list, list, g, j0, j1, k, 0u, at);
		T e[kExactBatch];
#pragma unroll
		for (uint32_t i = 0; i < kExactBatch; ++i) { e[i] = sorted_list_at<VB, GLOBAL>(s_list, list, g, at[i]); }
#pragma unroll
		for (uint32_t i = 0; i < kExactBatch; ++i) {
			const uint32_t idx = at[i] < last_key ? at[i] : last_key; // the element sorted_list_at read
			const uint64_t w   = readlane64(sel, b + i);
			const uint64_t m   = w & ballot64(e[i] == k[i]);
			unmatched += static_cast<uint32_t>(__builtin_popcountll(w & ~m));
			const uint32_t what = kexact_step(a.table, a.counts, m, idx, static_cast<double>(q[i]), lane);
#pragma unroll
			for (uint32_t s = 1; s < 3u; ++s) { steps[s] += what == s ? 1u : 0u; }
		}
	}
	if (counted && unmatched != 0u && lane == 0u) { kexact_count(a.counts, g.n_list, unmatched); }
	return kVectorDecoded;
}

template <int VB, bool GLOBAL>
__global__ __launch_bounds__(kInThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_keyed_sum_exact(const ColumnStreams cv, const ColumnStreams ck, const InArgs g, const KeyedExactArgs a) {
	typedef typename DecodeVec<VB>::T T;
	__shared__ T        s_list[kInLdsBytes / VB];
	__shared__ uint64_t s_exc[kInWaves][2][16]; // per wavefront and column: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;

	// 0. the keys (GLOBAL: their pivots) into LDS, once per workgroup; the one workgroup barrier of the kernel
	sorted_list_stage<VB, GLOBAL>(s_list, static_cast<const T*>(g.list), g);
	__syncthreads();

	const uint64_t n_waves  = static_cast<uint64_t>(gridDim.x) * kInWaves;
	uint32_t       did[4]   = {0u, 0u, 0u, 0u};
	uint32_t       steps[3] = {0u, 0u, 0u};
	for (uint64_t v = static_cast<uint64_t>(blockIdx.x) * kInWaves + wave; v < a.n_vectors; v += n_waves) {
		const uint32_t what = kexact_vector<VB, GLOBAL>(cv, ck, g, a, v, wave, lane, s_list, s_exc, steps);
#pragma unroll
		for (uint32_t i = 0; i < 4u; ++i) { did[i] += what == i ? 1u : 0u; }
	}
	if (a.trace != nullptr && lane < 6u) { // the trace: one add per wavefront and counter
		const uint32_t mine = lane == 0u ? did[0] : lane == 1u ? did[1] : lane == 2u ? did[2] : lane == 3u ? did[3] : lane == 4u ? steps[1] : steps[2];
		if (mine != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(a.trace) + lane, static_cast<unsigned long long>(mine)); }
	}
}

// n_pairs 16-byte pairs of the table and n_counts words of the counts (nullable) zeroed
__global__ __launch_bounds__(256) void k_keyed_exact_zero(ulonglong2* table, uint64_t n_pairs, uint64_t* counts, uint32_t n_counts) {
	const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
	const uint64_t t      = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
	for (uint64_t i = t; i < n_pairs; i += stride) { table[i] = make_ulonglong2(0ull, 0ull); }
	if (counts != nullptr) {
		for (uint64_t i = t; i < n_counts; i += stride) { counts[i] = 0ull; }
	}
}

// sums[i] = key i's entry rounded once
__global__ __launch_bounds__(256) void k_keyed_sum_exact_finish(const int64_t* __restrict__ table, uint32_t n_keys, double* __restrict__ sums) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_keys) { return; }
	const int64_t* entry = table + static_cast<uint64_t>(i) * kExactKeyWords;
	sums[i]              = __longlong_as_double(static_cast<long long>(exact_round_limbs_bits(entry, static_cast<uint64_t>(entry[kExactLimbs]))));
}

template <int VB>
static int launch_exact_vb(hipStream_t stream, const ColumnStreams& cv, const ColumnStreams& ck, const InArgs& g, const KeyedExactArgs& a, unsigned grid) {
	if (g.stride > 1u) {
		hipLaunchKernelGGL((k_keyed_sum_exact<VB, true>), dim3(grid), dim3(kInThreads), 0, stream, cv, ck, g, a);
	} else {
		hipLaunchKernelGGL((k_keyed_sum_exact<VB, false>), dim3(grid), dim3(kInThreads), 0, stream, cv, ck, g, a);
	}
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

uint64_t keyed_sum_exact_table_bytes(uint32_t n_keys) { return (static_cast<uint64_t>(n_keys) * kExactKeyWords * 8ull + 15ull) & ~15ull; }

// val->n_vectors == key->n_vectors in 0 .. ALPGPU_KEYED_EXACT_VECTORS_MAX (0: neither column is read), n_keys in 1 .. ALPGPU_KEYED_MANY_KEYS_MAX, the
// alignments checked by the caller.  The zero kernel unless accumulate, one launch of persistent workgroups unless there is no vector, the finish kernel.
int launch_keyed_sum_exact(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_keys,
                           uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_table, int accumulate, int value_bytes, int n_cus, const alpgpu_keyed_tuning* tuning,
                           uint64_t* d_trace) {
	if (!accumulate) {
		const uint64_t n_pairs = keyed_sum_exact_table_bytes(n_keys) / 16ull;
		const uint64_t blocks  = (n_pairs + 255ull) / 256ull;
		const unsigned grid    = static_cast<unsigned>(blocks < 16384ull ? blocks : 16384ull);
		hipLaunchKernelGGL(k_keyed_exact_zero, dim3(grid), dim3(256), 0, stream, static_cast<ulonglong2*>(d_table), n_pairs, d_counts, n_keys + 1u);
		if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	}
	if (val->n_vectors > 0) {
		KeyedExactArgs a {};
		a.n_vectors = val->n_vectors;
		a.mask      = d_mask;
		a.table     = static_cast<int64_t*>(d_table);
		a.counts    = d_counts;
		a.trace     = d_trace;
		const ListStaging staging = list_staging(n_keys, value_bytes);
		InArgs            g {};
		g.list   = d_keys;
		g.zones  = d_zones;
		g.n_list = n_keys;
		g.stride = staging.stride;
		g.n_piv  = staging.n_piv;
		const unsigned      grid = persistent_grid(val->n_vectors, kInWaves, n_cus, kExactWgPerCu, 0, tuning != nullptr ? tuning->grid : 0u, kTuningGridMax);
		const ColumnStreams cv = column_streams(val), ck = column_streams(key);
		const int           rc = value_bytes == 8 ? launch_exact_vb<8>(stream, cv, ck, g, a, grid) : launch_exact_vb<4>(stream, cv, ck, g, a, grid);
		if (rc != ALPGPU_OK) { return rc; }
	}
	hipLaunchKernelGGL(k_keyed_sum_exact_finish, dim3((n_keys + 255u) / 256u), dim3(256), 0, stream, static_cast<const int64_t*>(d_table), n_keys, d_sums);
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

} // namespace alpgpu
