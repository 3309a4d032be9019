// top_k_device.hpp — top-k (include/alpgpu.h, "top-k": alpgpu_top_k_*): the order, the composite keys, the state of the radix select and
// k_top_k_candidates, on the in-register decode of register_decode.hpp (batches of kStepBatch steps) and the skeleton of k_minmax_masked.
// Everything that is counted is an integer and everything that is compared is a unique key, so the result is a function of the inputs alone.
//
// The order (include/alpgpu.h): okey(x) = bits ^ (sign ? all-ones : sign-bit), an unsigned monotone bijection on the bits of the values that are
// not NaNs: -inf < ... < -0.0 < +0.0 < ... < +inf.  An element's composite key is {hi, lo} = {okey(x), ~index} for `largest` and
// {~okey(x), ~index} for smallest (hi within the value's width, zero-extended): descending composite order is the result's order, no two
// elements of a column share a key, and the value's bits come back out of hi.  A vector's key is {hi of its record's max (min), ~v}.
#pragma once
#include "register_decode.hpp"

namespace alpgpu {

constexpr int      kTopKHistThreads = 256;
constexpr unsigned kTopKHistGrid    = 256; // workgroups of a histogram pass at most: 256 integer atomics each
constexpr uint32_t kTopKMaxPasses   = 16;  // digits of a level at most: 8 of the key and 8 of the index
constexpr uint32_t kTopKSortMax     = ALPGPU_TOP_K_MAX;

// What a radix select has settled so far, in device memory: one record per level (0: vectors, 1: elements).  Zeroed by the call's memset;
// the pick of a level's first pass sets rank and count.
struct TopKState {
	uint64_t thr_hi, thr_lo; // the digits settled so far of the key looked for, the rest zero; after the last pass: the threshold
	uint32_t rank;           // the key looked for is the rank-th largest of those that match the settled digits (1-based)
	uint32_t count;          // min(k, keys there are): how many keys lie at or above the threshold.  0: there is none
	uint32_t n_items;        // level 1: candidates appended (may pass the capacity: readers clamp)
	uint32_t n_stage;        // level 1: staging slots taken (may pass k: the writers clamp)
};

// one pass of a select, fixed on the host: the digit is bits [shift, shift + 8) of hi (lo), and a key takes part if it equals the threshold under
// the masks (the digits settled by the passes before)
struct TopKPass {
	uint64_t mask_hi, mask_lo;
	uint64_t fill_lo; // the bits of lo above the index's bytes: ones in every key, so no pass visits them and the first pick sets them
	uint32_t shift;
	uint32_t in_lo; // 0: a digit of hi, 1: of lo
	uint32_t first; // the level's first pass: the pick starts from k
	uint32_t k;
};

template <int VB>
__device__ __forceinline__ uint64_t top_k_okey(typename DecodeVec<VB>::T x) {
	if constexpr (VB == 8) {
		const uint64_t b = static_cast<uint64_t>(__double_as_longlong(x));
		return b ^ (static_cast<uint64_t>(static_cast<int64_t>(b) >> 63) | 0x8000000000000000ull);
	} else {
		const uint32_t b = __float_as_uint(x);
		return b ^ (static_cast<uint32_t>(static_cast<int32_t>(b) >> 31) | 0x80000000u);
	}
}
template <int VB>
__device__ __forceinline__ bool top_k_is_nan(typename DecodeVec<VB>::T x) {
	if constexpr (VB == 8) {
		return (static_cast<uint64_t>(__double_as_longlong(x)) & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
	} else {
		return (__float_as_uint(x) & 0x7FFFFFFFu) > 0x7F800000u;
	}
}
// hi of a value's composite key
template <int VB>
__device__ __forceinline__ uint64_t top_k_hi(typename DecodeVec<VB>::T x, bool largest) {
	const uint64_t o = top_k_okey<VB>(x);
	return largest ? o : (VB == 8 ? ~o : (~o & 0xFFFFFFFFull));
}
// ... and the value's bits back out of it
template <int VB>
__device__ __forceinline__ uint64_t top_k_bits_of_hi(uint64_t hi, bool largest) {
	const uint64_t all  = VB == 8 ? ~0ull : 0xFFFFFFFFull;
	const uint64_t sign = VB == 8 ? 0x8000000000000000ull : 0x80000000ull;
	const uint64_t o    = largest ? hi : (~hi & all);
	return o & sign ? o ^ sign : (~o & all);
}
__device__ __forceinline__ bool top_k_at_or_above(uint64_t hi, uint64_t lo, uint64_t thr_hi, uint64_t thr_lo) { return hi > thr_hi || (hi == thr_hi && lo >= thr_lo); }

// record v as {min, max}; a vector is empty when min > max (what k_minmax_masked writes for nothing selected or nothing but NaNs)
template <int VB>
__device__ __forceinline__ bool top_k_record(const void* zones, uint64_t v, bool largest, uint64_t& hi) {
	typename DecodeVec<VB>::T mn, mx;
	if constexpr (VB == 8) {
		const double2 z = static_cast<const double2*>(zones)[v];
		mn = z.x, mx = z.y;
	} else {
		const float2 z = static_cast<const float2*>(zones)[v];
		mn = z.x, mx = z.y;
	}
	hi = top_k_hi<VB>(largest ? mx : mn, largest);
	return !(mn > mx);
}

struct TopKCandArgs {
	uint64_t         n_vectors, wg_off; // the launch covers the whole column, this grid from workgroup wg_off on
	const uint64_t*  mask;              // only read
	const void*      zones;             // the records, the caller's or the call's own
	const TopKState* vec;               // the vector level's threshold Tv
	TopKState*       elem;              // n_items: the candidates appended
	uint64_t*        cand;              // [capacity] pairs {hi, lo}
	uint32_t         capacity;          // min(k, n_vectors) * 1024
	uint32_t         k;
	int              largest;
};

// One wavefront per vector, four per workgroup, sharing nothing.  A vector below Tv costs its record and the threshold; a kept one is decoded in
// registers, and the values whose bit is set, that are no NaN and whose key reaches the value part of Tv are appended to the candidates, kStepBatch steps
// at a time: one atomic add per batch and wavefront of the batch's ballot popcounts, the slot of a lane from mbcnt.  Every slot is clamped
// against the capacity, so records that lie cannot make the kernel write outside the array.
template <int VB>
__global__ __launch_bounds__(kSelThreads) void k_top_k_candidates(const ColumnStreams c, const TopKCandArgs g) {
	typedef typename DecodeVec<VB>::T T;
	__shared__ uint64_t             s_exc[kSelWaves][16]; // per wavefront: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t v    = (g.wg_off + blockIdx.x) * kSelWaves + wave;
	if (v >= g.n_vectors) { return; }
	const bool largest = g.largest != 0;

	// 1. the record against Tv: 16 bytes, and nothing else for a vector that is not kept
	const uint32_t kept = g.vec->count;
	if (kept == 0u) { return; }
	uint64_t rec_hi;
	if (!top_k_record<VB>(g.zones, v, largest, rec_hi) || !top_k_at_or_above(rec_hi, ~v, g.vec->thr_hi, g.vec->thr_lo)) { return; }
	// k kept vectors hold k values that reach the value part of Tv, so nothing below it can win; fewer than k (every non-empty vector is kept) hold
	// no such promise, and every selected value is a candidate
	const uint64_t thr_hi = kept < g.k ? 0ull : g.vec->thr_hi;

	// 2. the vector's 128 bytes of bitmap, lane m < 16 holding word m (records that lie may keep a vector without a set bit)
	uint64_t prior;
	if (!bitmap_words(g.mask, v, lane, prior)) { return; }

	// 3. the descriptor and dictionary, the exception mask
	const DecodeVec<VB> A = decode_vec_load<VB>(c, v);
	exception_mask(A, s_exc, wave, lane);

	uint32_t exc_a = 0; // exceptions of the steps done
	for (uint32_t b = 0; b < 16u; b += kStepBatch) {
		// 4. every load of kStepBatch steps is requested before the first is used
		StepBatch<VB, kStepBatch> Ra;
		step_request(A, s_exc[wave], b, lane, exc_a, Ra);
		// 5. the batch's keys and who keeps one
		uint64_t hi[kStepBatch], keep[kStepBatch];
		uint32_t total = 0;
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			const T        x = step_value(A, Ra, b, i, lane);
			const uint64_t w = readlane64(prior, b + i);
			hi[i]            = top_k_hi<VB>(x, largest);
			keep[i]          = w & ballot64(!top_k_is_nan<VB>(x)) & ballot64(hi[i] >= thr_hi);
			total += static_cast<uint32_t>(__builtin_popcountll(keep[i]));
		}
		if (total == 0u) { continue; } // (wave-uniform)
		// 6. one atomic add for the batch, then the stores
		uint32_t base = 0;
		if (lane == 0u) { base = atomicAdd(&g.elem->n_items, total); }
		base = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(base)));
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			const uint32_t slot = mbcnt64(keep[i], base);
			if (((keep[i] >> lane) & 1ull) && slot < g.capacity) {
				const uint64_t index = (v << 10) + 64u * (b + i) + lane;
				reinterpret_cast<ulonglong2*>(g.cand)[slot] = make_ulonglong2(hi[i], ~index);
			}
			base += static_cast<uint32_t>(__builtin_popcountll(keep[i]));
		}
	}
}

} // namespace alpgpu
