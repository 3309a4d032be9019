// pair_device.hpp — two columns decoded side by side by one wavefront: k_pair, the kernel behind the "two-column consumers" of include/alpgpu.h
// (alpgpu_compare_mask_*, alpgpu_decode_dot_masked_*).  Vector v of column A and vector v of column B are decoded in registers, step by step as
// k_select (select_device.hpp) decodes one — the same layout of the steps, the same exception mask, the same arithmetic and the same clamps on
// bw, lbw, e, f and exc_cnt — and combined lane by lane: compared, the ballot kept in the bitmap, or multiplied and added up under the bitmap.
// The decode of ONE vector is PairVec / PairBatch below, used twice; k_select itself is left as it is (its instruction stream is measured).
#pragma once
#include "select_device.hpp"

namespace alpgpu {

constexpr uint32_t kPairBatch = 4; // steps of a vector PAIR whose words are requested together: as many vector loads in flight as k_select's 8 steps of one
constexpr int      kPairCompare = 0, kPairDot = 1;
// what a comparison accepts, as bits over the four outcomes of a < b, a == b, a > b, unordered (a NaN on either side): the kernel knows these only
constexpr uint32_t kPairLt = 1u, kPairEq = 2u, kPairGt = 4u, kPairUn = 8u;

struct PairColumn { // the four streams of an alpgpu_column the decode follows
	const alpgpu_vector_desc*    descs;
	const alpgpu_rowgroup_state* rgs;
	const uint8_t*               packed;
	const uint8_t*               excs;
};
struct PairArgs {
	uint64_t  v0, n_range, wg_off; // the launch covers vectors v0 + [0, n_range), this grid from workgroup wg_off on
	uint64_t  first, end;          // compare: the selected index range
	uint64_t* mask;                // compare: combined and stored; dot: only read
	double*   sums;                // dot
	uint32_t* counts;              // dot, nullable
	int       op;                  // compare: kMaskSet / kMaskAnd / kMaskOr
	uint32_t  accept;              // compare: kPairLt | kPairEq | kPairGt | kPairUn
};

// one vector's constants: everything wave-uniform
template <int VB>
struct PairVec {
	typedef typename std::conditional<VB == 8, uint64_t, uint32_t>::type U;
	typedef typename std::conditional<VB == 8, double, float>::type      T;
	const U*        words;
	const uint16_t* lefts;
	const uint8_t*  rec;
	U               base;
	uint32_t        bw, lbw, cnt;
	bool            alp;
	RdDict          dict;
	typename std::conditional<VB == 8, int64_t, uint32_t>::type fact;
	T                                                          frac;
	const uint16_t*                                            pos; // the exception positions
};

template <int VB>
__device__ __forceinline__ PairVec<VB> pair_vec_load(const PairColumn& c, uint64_t v) {
	typedef typename PairVec<VB>::U U;
	const alpgpu_vector_desc d = c.descs[v];
	PairVec<VB>              V;
	V.alp   = d.scheme == ALPGPU_SCHEME_ALP;
	V.bw    = d.bw < 8u * VB ? d.bw : 8u * VB;
	V.cnt   = d.exc_cnt < 1024u ? d.exc_cnt : 1024u;
	V.rec   = c.excs + d.exc_off;
	V.words = reinterpret_cast<const U*>(c.packed + d.packed_off);
	V.lefts = reinterpret_cast<const uint16_t*>(c.packed + d.packed_off + 128ull * d.bw);
	V.base  = static_cast<U>(d.base);
	V.lbw   = d.lbw < 16u ? d.lbw : 16u;
	const uint32_t fi = VB == 8 ? (d.f < 18 ? d.f : 18) : (d.f < 10 ? d.f : 10);
	const uint32_t ei = VB == 8 ? (d.e < 20 ? d.e : 20) : (d.e < 10 ? d.e : 10);
	V.dict            = load_rd_dict(c.rgs, v, !V.alp);
	if constexpr (VB == 8) {
		V.fact = kFactArr[fi];
		V.frac = kFracArr[ei];
	} else {
		V.fact = kFactArrF[fi];
		V.frac = kFracArrF[ei];
	}
	V.pos = reinterpret_cast<const uint16_t*>(V.rec + (V.alp ? static_cast<uint64_t>(VB) : 2ull) * d.exc_cnt);
	return V;
}

// the vector's exception positions into its 16 words of LDS (zeroed, and synchronised on both sides, by the caller)
template <int VB>
__device__ __forceinline__ void pair_mark_exceptions(const PairVec<VB>& V, uint64_t* s_words, uint32_t lane) {
	for (uint32_t j = lane; j < V.cnt; j += 64u) {
		const uint32_t q = V.pos[j];
		if (q < 1024u) { atomicOr(reinterpret_cast<uint32_t*>(s_words) + (q >> 5), 1u << (q & 31u)); }
	}
}

// what kPairBatch steps of one vector need from memory
template <int VB>
struct PairBatch {
	typedef typename PairVec<VB>::U U;
	FieldWords<U>        rw[kPairBatch];
	FieldWords<uint16_t> lw[kPairBatch];
	uint64_t             em[kPairBatch]; // wave-uniform: bit l = value 64 m + l is an exception
	U                    ev[kPairBatch];
};

// requests steps b .. b + kPairBatch - 1: the packed words, the ALP_RD left words and the exception values by rank; nothing is waited for here.
// before_exc: the vector's exceptions in the steps done, moved on
template <int VB>
__device__ __forceinline__ void pair_request(const PairVec<VB>& V, const uint64_t* s_words, uint32_t b, uint32_t lane, uint32_t& before_exc, PairBatch<VB>& R) {
	typedef typename PairVec<VB>::U U;
	constexpr uint32_t kLanes = VB == 8 ? 16u : 32u; // FastLanes lanes of the value streams
	constexpr uint32_t kLog   = VB == 8 ? 4u : 5u;
#pragma unroll
	for (uint32_t i = 0; i < kPairBatch; ++i) {
		R.rw[i] = FieldWords<U> {0, 0};
		R.lw[i] = FieldWords<uint16_t> {0, 0};
		R.em[i] = 0ull;
		R.ev[i] = 0;
	}
	if (V.bw > 0) {
#pragma unroll
		for (uint32_t i = 0; i < kPairBatch; ++i) {
			const uint32_t p = 64u * (b + i) + lane;
			R.rw[i]          = load_field_words<U, kLanes>(V.words + (p & (kLanes - 1u)), p >> kLog, V.bw);
		}
	}
	if (!V.alp && V.lbw > 0) {
#pragma unroll
		for (uint32_t i = 0; i < kPairBatch; ++i) { R.lw[i] = load_field_words<uint16_t, 64>(V.lefts + lane, b + i, V.lbw); }
	}
	if (V.cnt > 0) {
		uint32_t rank0 = before_exc;
#pragma unroll
		for (uint32_t i = 0; i < kPairBatch; ++i) {
			const uint64_t w    = s_words[b + i];
			const uint32_t w_lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(w)));
			const uint32_t w_hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(w >> 32)));
			R.em[i]             = (static_cast<uint64_t>(w_hi) << 32) | w_lo;
			const uint32_t rank = rank0 + mbcnt64(R.em[i], 0u);
			if ((R.em[i] >> lane) & 1ull) { R.ev[i] = V.alp ? reinterpret_cast<const U*>(V.rec)[rank] : static_cast<U>(reinterpret_cast<const uint16_t*>(V.rec)[rank]); }
			rank0 += static_cast<uint32_t>(__builtin_popcountll(R.em[i]));
		}
		before_exc = rank0;
	}
}

// value 64 (b + i) + lane of the vector, bit for bit what the store decode writes there
template <int VB>
__device__ __forceinline__ typename PairVec<VB>::T pair_value(const PairVec<VB>& V, const PairBatch<VB>& R, uint32_t b, uint32_t i, uint32_t lane) {
	typedef typename PairVec<VB>::U U;
	constexpr uint32_t kLog  = VB == 8 ? 4u : 5u;
	const uint32_t     m     = b + i;
	const uint32_t     p     = 64u * m + lane;
	const U            right = extract_field<U>(R.rw[i], p >> kLog, V.bw); // ALP: the digit; ALP_RD: the right part
	const bool         hit   = (R.em[i] >> lane) & 1ull;
	U                  bits;
	if (V.alp) {
		if constexpr (VB == 8) {
			bits = static_cast<U>(__double_as_longlong(decode_value(static_cast<int64_t>(right + V.base), V.fact, V.frac)));
		} else {
			bits = __float_as_uint(decode_value_f32(static_cast<int32_t>(right + V.base), V.fact, V.frac));
		}
		bits = hit ? R.ev[i] : bits;
	} else {
		const uint32_t idx  = extract_field<uint16_t>(R.lw[i], m, V.lbw) & 7u;
		const U        left = hit ? R.ev[i] : static_cast<U>(((idx < 4u ? V.dict.lo : V.dict.hi) >> (16u * (idx & 3u))) & 0xFFFFull);
		bits                = static_cast<U>((left << V.bw) | right);
	}
	if constexpr (VB == 8) { return __longlong_as_double(static_cast<long long>(bits)); } else { return __uint_as_float(bits); }
}

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
__global__ __launch_bounds__(kSelThreads) void k_pair(const PairColumn ca, const PairColumn cb, const PairArgs g) {
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
		uint64_t*  mw      = g.mask + 16ull * v;
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
		p_begin = g.first > r0 ? static_cast<uint32_t>(g.first - r0) : 0u; // the vector's share of [first, end): wave-uniform
		p_end   = g.end - r0 < 1024u ? static_cast<uint32_t>(g.end - r0) : 1024u;
	} else {
		prior = lane < 16u ? static_cast<const uint64_t*>(g.mask)[16ull * v + lane] : 0ull;
		if (ballot64(prior != 0ull) == 0ull) {
			if (lane == 0u) {
				g.sums[v] = 0.0;
				if (g.counts != nullptr) { g.counts[v] = 0u; }
			}
			return;
		}
	}

	// 2. both descriptors and dictionaries
	const PairVec<VB> A = pair_vec_load<VB>(ca, v);
	const PairVec<VB> B = pair_vec_load<VB>(cb, v);

	// 3. both exception masks
	if ((A.cnt | B.cnt) > 0) {
		if (lane < 32u) { s_exc[wave][lane >> 4][lane & 15u] = 0ull; }
		wave_lds_sync();
		pair_mark_exceptions<VB>(A, s_exc[wave][0], lane);
		pair_mark_exceptions<VB>(B, s_exc[wave][1], lane);
		wave_lds_sync();
	}

	uint32_t exc_a = 0, exc_b = 0; // exceptions of the steps done
	uint32_t n_set = 0;            // dot: set bits of the steps done
	uint64_t keep  = 0;            // compare: lane m < 16 keeps step m's ballot
	double   acc   = 0.0;          // dot: this lane's partial
	for (uint32_t b = 0; b < 16u; b += kPairBatch) {
		// 4. every load of kPairBatch steps of BOTH vectors is requested before the first is used
		PairBatch<VB> Ra, Rb;
		pair_request<VB>(A, s_exc[wave][0], b, lane, exc_a, Ra);
		pair_request<VB>(B, s_exc[wave][1], b, lane, exc_b, Rb);
#pragma unroll
		for (uint32_t i = 0; i < kPairBatch; ++i) {
			const uint32_t m = b + i;
			// 5. the two values
			const typename PairVec<VB>::T xa = pair_value<VB>(A, Ra, b, i, lane);
			const typename PairVec<VB>::T xb = pair_value<VB>(B, Rb, b, i, lane);
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
