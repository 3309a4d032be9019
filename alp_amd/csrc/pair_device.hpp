// pair_device.hpp — two columns decoded side by side by one wavefront: k_pair, the kernel behind the "two-column consumers" of include/alpgpu.h
// (alpgpu_compare_mask_*, alpgpu_decode_dot_masked_*).  Vector v of column A and vector v of column B are decoded in registers by
// register_decode.hpp, kStepBatch steps of both at a time, and combined lane by lane: compared, the ballot kept in the bitmap, or multiplied and
// added up under the bitmap.
#pragma once
#include "register_decode.hpp"

namespace alpgpu {

constexpr int kPairCompare = 0, kPairDot = 1;
// what a comparison accepts, as bits over the four outcomes of a < b, a == b, a > b, unordered (a NaN on either side): the kernel knows these only
constexpr uint32_t kPairLt = 1u, kPairEq = 2u, kPairGt = 4u, kPairUn = 8u;

struct PairArgs {
	uint64_t  v0, n_range, wg_off; // the launch covers vectors v0 + [0, n_range), this grid from workgroup wg_off on
	uint64_t  first, end;          // compare: the selected index range
	uint64_t* mask;                // compare: combined and stored; dot: only read
	double*   sums;                // dot
	uint32_t* counts;              // dot, nullable
	int       op;                  // compare: kMaskSet / kMaskAnd / kMaskOr
	uint32_t  accept;              // compare: kPairLt | kPairEq | kPairGt | kPairUn
};

// acc + a * b as two operations, each rounded once: the product is formed, kept from the optimiser's sight, and then added.  The library is built
// with -ffp-contract=off, and the pragma says the same for this function under any flag; the empty asm is what makes a fused multiply-add
// impossible whatever the compiler is told, since the add's operand is no longer known to be a product.
__device__ __forceinline__ double pair_mul_then_add(double acc, double a, double b) {
#pragma clang fp contract(off)
	double t = a * b;
	asm volatile("" : "+v"(t));
	return acc + t;
}

// One wavefront per vector pair, four per workgroup, sharing nothing.  ARM = kPairCompare: alpgpu_compare_mask_*; kPairDot: alpgpu_decode_dot_masked_*.
template <int VB, int ARM>
__global__ __launch_bounds__(kSelThreads) void k_pair(const ColumnStreams ca, const ColumnStreams cb, const PairArgs g) {
	__shared__ uint64_t s_exc[kSelWaves][2][16]; // per wavefront and column: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t k    = (g.wg_off + blockIdx.x) * kSelWaves + wave;
	if (k >= g.n_range) { return; }
	const uint64_t v  = g.v0 + k;
	const uint64_t r0 = v << 10;

	// 1. the vector's 128 bytes of bitmap, lane m < 16 holding word m, and what they settle without the columns
	uint64_t prior   = 0;
	uint32_t p_begin = 0, p_end = 1024u;
	if constexpr (ARM == kPairCompare) {
		uint64_t* mw = g.mask + 16ull * v;
		// (written out in each of the three kernels that write a bitmap, and not a helper: the note at the end of register_decode.hpp)
		const bool outside = r0 >= g.end || r0 + 1024u <= g.first; // no value of the vector is in the range: q is false throughout
		if (g.op == kMaskSet) {
			if (outside) {
				if (lane < 16u) { mw[lane] = 0ull; }
				return;
			}
		} else {
			const uint64_t neutral = g.op == kMaskAnd ? 0ull : ~0ull; // the word that q cannot change
			prior                  = lane < 16u ? mw[lane] : neutral;
			if (ballot64(prior != neutral) == 0ull) { return; } // AND of all zeros, OR of all ones: these 128 bytes were all that was read
			if (outside) {
				if (g.op == kMaskAnd && lane < 16u) { mw[lane] = 0ull; }
				return;
			}
		}
		range_share(g.first, g.end, r0, p_begin, p_end);
	} else {
		if (!bitmap_words(g.mask, v, lane, prior)) {
			if (lane == 0u) {
				g.sums[v] = 0.0;
				if (g.counts != nullptr) { g.counts[v] = 0u; }
			}
			return;
		}
	}

	// 2. both descriptors and dictionaries, 3. both exception masks
	const DecodeVec<VB> A = decode_vec_load<VB>(ca, v);
	const DecodeVec<VB> B = decode_vec_load<VB>(cb, v);
	exception_masks(A, B, s_exc, wave, lane);

	uint32_t exc_a = 0, exc_b = 0; // exceptions of the steps done
	uint32_t n_set = 0;            // dot: set bits of the steps done
	uint64_t keep  = 0;            // compare: lane m < 16 keeps step m's ballot
	double   acc   = 0.0;          // dot: this lane's partial
	for (uint32_t b = 0; b < 16u; b += kStepBatch) {
		// 4. every load of kStepBatch steps of BOTH vectors is requested before the first is used
		StepBatch<VB, kStepBatch> Ra, Rb;
		step_request(A, s_exc[wave][0], b, lane, exc_a, Ra);
		step_request(B, s_exc[wave][1], b, lane, exc_b, Rb);
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			const uint32_t m = b + i;
			// 5. the two values
			const typename DecodeVec<VB>::T xa = step_value(A, Ra, b, i, lane);
			const typename DecodeVec<VB>::T xb = step_value(B, Rb, b, i, lane);
			// 6. compared or accumulated
			if constexpr (ARM == kPairCompare) {
				const uint32_t p  = 64u * m + lane;
				const uint64_t in = ballot64(p - p_begin < p_end - p_begin); // p_begin <= p < p_end
				const uint64_t lt = ballot64(xa < xb), eq = ballot64(xa == xb), gt = ballot64(xa > xb); // C's comparisons: all false with a NaN; -0.0 == 0.0
				uint64_t       sel = (g.accept & kPairLt ? lt : 0ull) | (g.accept & kPairEq ? eq : 0ull) | (g.accept & kPairGt ? gt : 0ull) | (g.accept & kPairUn ? ~(lt | eq | gt) : 0ull);
				sel &= in;
				keep = lane == m ? sel : keep;
			} else {
				const uint64_t w = readlane64(prior, m);
				if ((w >> lane) & 1ull) { acc = pair_mul_then_add(acc, static_cast<double>(xa), static_cast<double>(xb)); }
				n_set += static_cast<uint32_t>(__builtin_popcountll(w));
			}
		}
	}
	if constexpr (ARM == kPairCompare) {
		if (lane < 16u) { g.mask[16ull * v + lane] = g.op == kMaskAnd ? (prior & keep) : g.op == kMaskOr ? (prior | keep) : keep; } // one run of 128 bytes
	} else {
		const double total = wave_tree_sum_f64(acc);
		if (lane == 0u) {
			g.sums[v] = total;
			if (g.counts != nullptr) { g.counts[v] = n_set; }
		}
	}
}

} // namespace alpgpu
