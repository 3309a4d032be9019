// select_device.hpp — the one-wavefront decode of a vector that every kernel of the selection family is an arm of: k_select, shared by
// select_kernels.hip (count, zoned count, emit) and mask_kernels.hip (ballots kept as a bitmap, masked SUM, masked projection).  The layout of the steps, the
// exception mask and the arithmetic are described at the head of select_kernels.hip.
#pragma once
#include <type_traits>

#include "alp_device_f32.hpp"
#include "lane_field.hpp"
#include "launch.hpp"

namespace alpgpu {

constexpr int      kSelWaves   = 4; // wavefronts per workgroup, one vector each (they share nothing)
constexpr int      kSelThreads = 64 * kSelWaves;
constexpr uint64_t kSelMaxGrid = 1ull << 30; // workgroups per launch
constexpr int      kScanBlock  = 1024;       // counts per scan block = threads per scan workgroup
constexpr uint32_t kSelBatch   = 8;          // steps of a vector whose words are requested together
inline uint64_t    align16(uint64_t x) { return (x + 15ull) & ~15ull; } // the parts of the scratch (select_scratch_bytes) begin on 16 bytes

// EMIT = false: counts[k] = qualifying values of vector v0 + k.  EMIT = true: their indices (and values) at offsets[k] + rank.
// [first, end) is the selected index range; the launch covers exactly the vectors it touches (v0 = first >> 10, n_range of them).
// ZONES: empty, or one `const void*` behind the other arguments = the zoned count pass of alpgpu_select_range_zoned_*: zones[v] = {min, max} (one
// record per vector of the COLUMN, indexed by v, not by v - v0) is read first.  A vector whose zone misses [lo, hi] is counted 0 and one whose
// zone lies inside it, and which cannot hold a NaN, is counted whole; neither has its packed words or exception record read.  (A trailing
// parameter pack and not a plain parameter: the unzoned instantiations keep their argument list and with it their instructions.)
// Three more arms take their arguments the same way (mask_kernels.hip; include/alpgpu.h, "selection bitmaps").  In all the launch covers vectors of
// the whole column (v0 = 0) and word 16 v + m of the bitmap is step m's ballot: bit `lane` = value index 1024 v + 64 m + lane.
//   SelMaskArgs  alpgpu_select_mask_*: the 16 ballots of a vector are not counted but kept, lane m < 16 holding step m's, combined with what the
//                bitmap held (op) and stored as one run of 128 bytes.  A vector outside [first, end), one whose words are all zero under AND and
//                one whose words are all ones under OR is settled from those 128 bytes: its descriptor is not read.
//   SelSumArgs   alpgpu_decode_sum_masked_*: no predicate; lane L adds the values 64 m + L whose bit is set, m ascending, from +0.0 (floats widened
//                first), and the 64 partials combine by wave_tree_sum_f64.  A vector whose words are all zero gets +0.0 and 0 and is not read.
//   SelTakeArgs  alpgpu_decode_masked_*: no predicate; the emit pass of a selection whose ballots are the bitmap's words.  counts[v] = the vector's
//                set bits and offsets[v] = the set bits of the vectors before (k_mask_count and the scan ran first); the value at a set bit goes to
//                d_vals (and its index to d_idx, nullable here) at offsets[v] + the set bits of the words before + those below the lane, under
//                the capacity.  A vector with counts[v] == 0 costs those four bytes, one at or behind the capacity its offset too; a batch of
//                kSelBatch steps whose words are all zero requests nothing of the column and only moves the exception rank on.
constexpr int kMaskSet = ALPGPU_MASK_SET, kMaskAnd = ALPGPU_MASK_AND, kMaskOr = ALPGPU_MASK_OR;
struct SelMaskArgs {
	uint64_t* mask;
	int       op;
};
struct SelSumArgs {
	const uint64_t* mask;
	double*         sums;
	uint32_t*       counts; // nullable
};
struct SelTakeArgs {
	const uint64_t* mask;
	const uint32_t* counts; // (the kernel's own `counts` is the count pass's output: this arm only reads)
};
template <class... ZONES> struct sel_arm { static constexpr int value = 0; };
template <> struct sel_arm<const void*> { static constexpr int value = 1; };
template <> struct sel_arm<SelMaskArgs> { static constexpr int value = 2; };
template <> struct sel_arm<SelSumArgs> { static constexpr int value = 3; };
template <> struct sel_arm<SelTakeArgs> { static constexpr int value = 4; };
__device__ __forceinline__ const void* zone_records(const void* zones) { return zones; }
template <class A> __device__ __forceinline__ const A& arm_args(const A& a) { return a; }
// lane `idx` (wave-uniform) of a 64-bit value
__device__ __forceinline__ uint64_t readlane64(uint64_t x, uint32_t idx) {
	const uint32_t l = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(x), idx));
	const uint32_t h = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(x >> 32), idx));
	return (static_cast<uint64_t>(h) << 32) | l;
}
template <int VB, bool EMIT, class... ZONES>
__global__ __launch_bounds__(kSelThreads) void k_select(const alpgpu_vector_desc* __restrict__ descs, const alpgpu_rowgroup_state* __restrict__ rgs,
                                                        const uint8_t* __restrict__ packed, const uint8_t* __restrict__ excs, uint64_t v0, uint64_t n_range,
                                                        uint64_t wg_off, uint64_t first, uint64_t end, double range_lo, double range_hi,
                                                        uint32_t* __restrict__ counts, const uint64_t* __restrict__ offsets, int64_t* __restrict__ d_idx,
                                                        void* __restrict__ d_vals, uint64_t capacity, ZONES... zones) {
	constexpr bool ZONED = sel_arm<ZONES...>::value == 1, MASK = sel_arm<ZONES...>::value == 2, SUM = sel_arm<ZONES...>::value == 3;
	constexpr bool TAKE = sel_arm<ZONES...>::value == 4;
	static_assert(sizeof...(ZONES) <= 1 && !((ZONED || MASK || SUM || TAKE) && EMIT), "at most one arm's arguments, and the emit pass reads the counts and nothing else");
	typedef typename std::conditional<VB == 8, uint64_t, uint32_t>::type U;
	typedef typename std::conditional<VB == 8, double, float>::type      T;
	constexpr uint32_t kLanes = VB == 8 ? 16u : 32u; // FastLanes lanes of the value streams
	constexpr uint32_t kLog   = VB == 8 ? 4u : 5u;
	__shared__ uint64_t s_exc[kSelWaves][16]; // per wavefront: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t k    = (wg_off + blockIdx.x) * kSelWaves + wave;
	if (k >= n_range) { return; }
	const uint64_t v       = v0 + k;
	const uint64_t r0      = v << 10;
	const uint32_t p_begin = first > r0 ? static_cast<uint32_t>(first - r0) : 0u; // the vector's share of [first, end): wave-uniform
	const uint32_t p_end   = end - r0 < 1024u ? static_cast<uint32_t>(end - r0) : 1024u;

	uint32_t total = 0;
	uint64_t out0  = 0;
	if constexpr (EMIT) {
		total = counts[k];
		if (total == 0) { return; } // a vector without a qualifying value costs these four bytes
		out0 = offsets[k];
		if (out0 >= capacity) { return; }
		if (d_vals == nullptr && total == p_end - p_begin) { // all of it qualifies and only indices are wanted: nothing to decode
			for (uint32_t p = p_begin + lane; p < p_end; p += 64u) {
				const uint64_t j = out0 + (p - p_begin);
				if (j < capacity) { d_idx[j] = static_cast<int64_t>(r0 + p); }
			}
			return;
		}
	}

	uint64_t prior = 0; // MASK, SUM, TAKE: lane m < 16 holds word m of the vector's bitmap as it was found
	if constexpr (MASK) {
		const SelMaskArgs& a       = arm_args(zones...);
		uint64_t*          mw      = a.mask + 16ull * v;
		const bool         outside = r0 >= end || r0 + 1024u <= first; // no value of the vector is in the range: q is false throughout
		if (a.op == kMaskSet) {
			if (outside) {
				if (lane < 16u) { mw[lane] = 0ull; }
				return;
			}
		} else {
			const uint64_t neutral = a.op == kMaskAnd ? 0ull : ~0ull; // the word that q cannot change
			prior                  = lane < 16u ? mw[lane] : neutral;
			if (ballot64(prior != neutral) == 0ull) { return; } // AND of all zeros, OR of all ones: these 128 bytes were all that was read
			if (outside) {
				if (a.op == kMaskAnd && lane < 16u) { mw[lane] = 0ull; }
				return;
			}
		}
	}
	if constexpr (SUM) {
		const SelSumArgs& a = arm_args(zones...);
		prior               = lane < 16u ? a.mask[16ull * v + lane] : 0ull;
		if (ballot64(prior != 0ull) == 0ull) {
			if (lane == 0u) {
				a.sums[v] = 0.0;
				if (a.counts != nullptr) { a.counts[v] = 0u; }
			}
			return;
		}
	}

	if constexpr (TAKE) {
		const SelTakeArgs& a = arm_args(zones...);
		total                = a.counts[v];
		if (total == 0) { return; } // a vector without a set bit costs these four bytes
		out0 = offsets[v];
		if (out0 >= capacity) { return; } // ... and one at or behind the capacity these eight more: its descriptor is not read
		prior = lane < 16u ? a.mask[16ull * v + lane] : 0ull; // one read of 128 bytes
	}

	bool inside = false; // ZONED: every value the zone admits qualifies
	if constexpr (ZONED) {
		const T* zone = reinterpret_cast<const T*>(zone_records(zones...)) + 2 * v; // (wave-uniform)
		const T  z_min = zone[0], z_max = zone[1];
		const T z_lo = static_cast<T>(range_lo), z_hi = static_cast<T>(range_hi);
		if (!(z_max >= z_lo && z_min <= z_hi)) { // excluded (a NaN bound excludes every vector): the record is all that was read
			if (lane == 0u) { counts[k] = 0u; }
			return;
		}
		inside = z_min >= z_lo && z_max <= z_hi;
	}
	const alpgpu_vector_desc d     = descs[v];
	const bool               alp   = d.scheme == ALPGPU_SCHEME_ALP;
	if constexpr (ZONED) {
		// contained: only a vector that cannot hold a NaN — ALP without exceptions (a NaN never round-trips through ALP, so it is always an exception)
		if (inside && alp && d.exc_cnt == 0u) {
			if (lane == 0u) { counts[k] = p_end - p_begin; }
			return;
		}
	}
	const uint32_t           bw    = d.bw < 8u * VB ? d.bw : 8u * VB;
	const uint32_t           cnt   = d.exc_cnt < 1024u ? d.exc_cnt : 1024u;
	const uint8_t*           rec   = excs + d.exc_off;
	const U*                 words = reinterpret_cast<const U*>(packed + d.packed_off);
	const uint16_t*          lefts = reinterpret_cast<const uint16_t*>(packed + d.packed_off + 128ull * d.bw);
	const U                  base  = static_cast<U>(d.base);
	// per-vector constants of the two schemes (gather_kernels.hip: value_bits reads the same tables with the same clamps)
	const uint32_t lbw  = d.lbw < 16u ? d.lbw : 16u;
	const uint32_t fi   = VB == 8 ? (d.f < 18 ? d.f : 18) : (d.f < 10 ? d.f : 10);
	const uint32_t ei   = VB == 8 ? (d.e < 20 ? d.e : 20) : (d.e < 10 ? d.e : 10);
	const RdDict   dict = load_rd_dict(rgs, v, !alp);
	const T        lo = static_cast<T>(range_lo), hi = static_cast<T>(range_hi);
	typename std::conditional<VB == 8, int64_t, uint32_t>::type fact;
	T                                                          frac;
	if constexpr (VB == 8) {
		fact = kFactArr[fi];
		frac = kFracArr[ei];
	} else {
		fact = kFactArrF[fi];
		frac = kFracArrF[ei];
	}

	if (cnt > 0) { // the exception positions as a mask in index order
		const uint16_t* pos = reinterpret_cast<const uint16_t*>(rec + (alp ? static_cast<uint64_t>(VB) : 2ull) * d.exc_cnt);
		if (lane < 16u) { s_exc[wave][lane] = 0ull; }
		wave_lds_sync();
		for (uint32_t j = lane; j < cnt; j += 64u) {
			const uint32_t q = pos[j];
			if (q < 1024u) { atomicOr(reinterpret_cast<uint32_t*>(&s_exc[wave][0]) + (q >> 5), 1u << (q & 31u)); }
		}
		wave_lds_sync();
	}

	uint32_t before_exc = 0; // exceptions of the steps done
	uint32_t before_sel = 0; // qualifying values of the steps done (wave-uniform: it comes from ballots); SUM, TAKE: set bits of the steps done
	uint64_t keep       = 0; // MASK: lane m < 16 keeps step m's ballot
	double   acc        = 0.0; // SUM: this lane's partial
	for (uint32_t b = 0; b < 16u; b += kSelBatch) {
		if constexpr (TAKE) {
			// no bit set in these kSelBatch words: nothing of the column is requested, but the exceptions of the steps passed over still count
			// towards the rank of those behind them
			if (ballot64(lane >= b && lane < b + kSelBatch && prior != 0ull) == 0ull) {
				if (cnt > 0) {
#pragma unroll
					for (uint32_t i = 0; i < kSelBatch; ++i) { before_exc += static_cast<uint32_t>(__builtin_popcountll(s_exc[wave][b + i])); } // (every lane reads the same word)
				}
				continue;
			}
		}
		// every load of kSelBatch steps is requested before the first is used: a step is otherwise its own round trip to memory
		FieldWords<U>        rw[kSelBatch];
		FieldWords<uint16_t> lw[kSelBatch];
#pragma unroll
		for (uint32_t i = 0; i < kSelBatch; ++i) {
			rw[i] = FieldWords<U> {0, 0};
			lw[i] = FieldWords<uint16_t> {0, 0};
		}
		if (bw > 0) {
#pragma unroll
			for (uint32_t i = 0; i < kSelBatch; ++i) {
				const uint32_t p = 64u * (b + i) + lane;
				rw[i]            = load_field_words<U, kLanes>(words + (p & (kLanes - 1u)), p >> kLog, bw);
			}
		}
		if (!alp && lbw > 0) {
#pragma unroll
			for (uint32_t i = 0; i < kSelBatch; ++i) { lw[i] = load_field_words<uint16_t, 64>(lefts + lane, b + i, lbw); }
		}
		// ... the exceptions' values too (ALP: the value's bits; ALP_RD: its left part): loaded where they are used, each step with an exception in
		// it would wait for memory once more.  (The ALP_RD loads are still waited for one by one in the generated code, see the head of this file.
		// A form that avoids it was measured: every lane loads, without the per-lane branch, one loop per scheme.  It takes 98 registers
		// instead of 81 and cost the mixed and float columns more, +4 % and +8 %, than the ALP_RD column gained, -3 %.)
		uint64_t em[kSelBatch]; // wave-uniform: bit l = value 64 m + l is an exception
		U        ev[kSelBatch];
#pragma unroll
		for (uint32_t i = 0; i < kSelBatch; ++i) {
			em[i] = 0ull;
			ev[i] = 0;
		}
		if (cnt > 0) {
			uint32_t rank0 = before_exc;
#pragma unroll
			for (uint32_t i = 0; i < kSelBatch; ++i) {
				const uint64_t w = s_exc[wave][b + i];
				const uint32_t w_lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(w))); // (the builtin returns int: no sign extension into the high word)
				const uint32_t w_hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(w >> 32)));
				em[i]               = (static_cast<uint64_t>(w_hi) << 32) | w_lo;
				const uint32_t rank = rank0 + mbcnt64(em[i], 0u);
				if ((em[i] >> lane) & 1ull) { ev[i] = alp ? reinterpret_cast<const U*>(rec)[rank] : static_cast<U>(reinterpret_cast<const uint16_t*>(rec)[rank]); }
				rank0 += static_cast<uint32_t>(__builtin_popcountll(em[i]));
			}
			before_exc = rank0;
		}
#pragma unroll
		for (uint32_t i = 0; i < kSelBatch; ++i) {
			const uint32_t m     = b + i;
			const uint32_t p     = 64u * m + lane;
			const U        right = extract_field<U>(rw[i], p >> kLog, bw); // ALP: the digit; ALP_RD: the right part
			const bool     hit   = (em[i] >> lane) & 1ull;
			U              bits;
			if (alp) {
				if constexpr (VB == 8) {
					bits = static_cast<U>(__double_as_longlong(decode_value(static_cast<int64_t>(right + base), fact, frac)));
				} else {
					bits = __float_as_uint(decode_value_f32(static_cast<int32_t>(right + base), fact, frac));
				}
				bits = hit ? ev[i] : bits;
			} else {
				const uint32_t idx  = extract_field<uint16_t>(lw[i], m, lbw) & 7u;
				const U        left = hit ? ev[i] : static_cast<U>(((idx < 4u ? dict.lo : dict.hi) >> (16u * (idx & 3u))) & 0xFFFFull);
				bits                = static_cast<U>((left << bw) | right);
			}
			T x;
			if constexpr (VB == 8) { x = __longlong_as_double(static_cast<long long>(bits)); } else { x = __uint_as_float(bits); }
			if constexpr (SUM) {
				const uint64_t w = readlane64(prior, m);
				if ((w >> lane) & 1ull) { acc += static_cast<double>(x); } // (an addition alone: nothing to contract)
				before_sel += static_cast<uint32_t>(__builtin_popcountll(w));
				continue;
			}
			if constexpr (TAKE) {
				const uint64_t w = readlane64(prior, m);
				const uint64_t j = out0 + before_sel + mbcnt64(w, 0u);
				if (((w >> lane) & 1ull) && j < capacity) { // (lanes of a dense word store side by side)
					reinterpret_cast<U*>(d_vals)[j] = bits;
					if (d_idx != nullptr) { d_idx[j] = static_cast<int64_t>(r0 + p); }
				}
				before_sel += static_cast<uint32_t>(__builtin_popcountll(w));
				continue;
			}
			const bool     q   = p >= p_begin && p < p_end && x >= lo && x <= hi; // NaN (value or bound) never qualifies; -0.0 == 0.0
			const uint64_t sel = ballot64(q);
			if constexpr (MASK) { keep = lane == m ? sel : keep; }
			if constexpr (EMIT) {
				const uint64_t j = out0 + before_sel + mbcnt64(sel, 0u);
				if (q && j < capacity) {
					d_idx[j] = static_cast<int64_t>(r0 + p);
					if (d_vals != nullptr) { reinterpret_cast<U*>(d_vals)[j] = bits; }
				}
			}
			before_sel += static_cast<uint32_t>(__builtin_popcountll(sel));
		}
		if constexpr (EMIT || TAKE) {
			if (before_sel >= total || out0 + before_sel >= capacity) { return; } // the vector's last qualifying value, or the capacity, is behind us
		}
	}
	if constexpr (MASK) {
		const SelMaskArgs& a = arm_args(zones...);
		if (lane < 16u) { a.mask[16ull * v + lane] = a.op == kMaskAnd ? (prior & keep) : a.op == kMaskOr ? (prior | keep) : keep; } // one run of 128 bytes
	} else if constexpr (SUM) {
		const SelSumArgs& a     = arm_args(zones...);
		const double      total_sum = wave_tree_sum_f64(acc);
		if (lane == 0u) {
			a.sums[v] = total_sum;
			if (a.counts != nullptr) { a.counts[v] = before_sel; }
		}
	} else if constexpr (!EMIT && !TAKE) {
		if (lane == 0u) { counts[k] = before_sel; }
	}
}

} // namespace alpgpu
