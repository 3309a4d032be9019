// register_decode.hpp — the in-register decode of one 1024-value vector by one wavefront, 64 lanes wide and step by step, and the glue its kernels
// share.  Every kernel of the selection family decodes through it: k_select (select_device.hpp: range selection, bitmaps, masked SUM and
// projection), k_pair (pair_device.hpp), k_group (group_device.hpp), k_minmax_masked and k_group_minmax (minmax_device.hpp), k_in_list
// (in_list_kernels.hip), k_join_probe (join_kernels.hip), k_top_k_candidates (top_k_device.hpp), k_quantile_wide (quantile_device.hpp),
// k_histogram (histogram_kernels.hip), k_distinct_insert (distinct_kernels.hip) and k_keyed_sum (keyed_kernels.hip).  A clamp or a layout rule of the
// decode is stated here and nowhere else; what the six persistent kernels among them share around it is stated once in persistent_scan.hpp (the selected bits, the
// constant-vector shortcut, the bin flush), sorted_list.hpp (a sorted list in LDS and its search) and persistent_launch.hpp (the host's grid and
// staging rules).
//
// The decode: 16 steps, step m holds value p = 64 m + lane in lane `lane`, so a wave-wide ballot of a predicate IS the 64 bits of the vector's
// qualify mask for indices 64 m .. 64 m + 63, in index order.  With p = 64 m + lane the lanes of a wavefront read neighbouring words of every
// stream (layouts: gather_kernels.hip):
//   ALP double   FastLanes lane p & 15 = lane & 15, row 4 m + (lane >> 4): four runs of 16 consecutive u64
//   ALP float    lane p & 31, row 2 m + (lane >> 5): two runs of 32 consecutive u32
//   ALP_RD left  lane p & 63 = lane, row m: 64 consecutive u16
// Exceptions: the record's ascending positions become a 1024-bit mask in the wavefront's 128 bytes of LDS (ds_or, as the store decode's
// ExcMask); step m reads its 64 bits, rank in the record = exceptions of the steps before + the mask's bits below the lane.  The arithmetic is
// the store decode's own (decode_value / decode_value_f32, the ALP_RD glue, the same tables and the same clamps as gather_kernels.hip's
// value_bits), so a value has the bits alpgpu_decode_* writes at its index.
//
// A kernel: DecodeVec (decode_vec_load), the exception mask (exception_mask, exception_masks), then per batch of NB steps step_request followed by
// step_bits / step_value of each step.  k_select takes 8 steps of one vector to a batch (kSelBatch), the others kStepBatch = 4 (of one vector or of
// two side by side: as many vector loads in flight).  Every one of them but k_in_list, k_join_probe, k_quantile_wide, k_histogram,
// k_distinct_insert and k_keyed_sum, which are persistent (their grid: persistent_launch.hpp), is launched by launch_vectors below.
#pragma once
#include <type_traits>

#include "alp_device_f32.hpp"
#include "lane_field.hpp"
#include "launch.hpp"

namespace alpgpu {

constexpr int      kSelWaves   = 4; // wavefronts per workgroup, one vector (or vector pair) each: they share nothing
constexpr int      kSelThreads = 64 * kSelWaves;
constexpr uint32_t kStepBatch  = 4; // steps of a vector whose words are requested together, for every kernel but k_select
constexpr int      kMaskSet = ALPGPU_MASK_SET, kMaskAnd = ALPGPU_MASK_AND, kMaskOr = ALPGPU_MASK_OR;

// lane `idx` (wave-uniform) of a 64-bit value
__device__ __forceinline__ uint64_t readlane64(uint64_t x, uint32_t idx) {
	const uint32_t l = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(x), idx));
	const uint32_t h = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<uint32_t>(x >> 32), idx));
	return (static_cast<uint64_t>(h) << 32) | l;
}

struct ColumnStreams { // the four streams of an alpgpu_column the decode follows
	const alpgpu_vector_desc*    descs;
	const alpgpu_rowgroup_state* rgs;
	const uint8_t*               packed;
	const uint8_t*               excs;
};
inline ColumnStreams column_streams(const alpgpu_column* col) { return ColumnStreams {col->d_vectors, col->d_rowgroups, col->d_packed, col->d_exc}; }

// The family's one launch loop (host side): n_vectors vectors, vectors_per_wg to a workgroup (kSelWaves: one wavefront per vector), split only at the
// grid limit (launch.hpp: grid_chunk).  launch(grid, wg_off) makes one chunk; the kernel takes wg_off, the chunk's first workgroup, as an argument.
template <class Launch>
inline int launch_vectors(uint64_t n_vectors, uint64_t vectors_per_wg, Launch&& launch) {
	const uint64_t n_wg = (n_vectors + vectors_per_wg - 1) / vectors_per_wg;
	for (uint64_t off = 0; off < n_wg; off += grid_chunk(n_wg - off)) {
		launch(dim3(static_cast<unsigned>(grid_chunk(n_wg - off))), off);
		if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	}
	return ALPGPU_OK;
}

// one vector's constants: everything wave-uniform, every field of the descriptor clamped to what its type admits
template <int VB>
struct DecodeVec {
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
__device__ __forceinline__ DecodeVec<VB> decode_vec_load(const ColumnStreams& c, uint64_t v) {
	typedef typename DecodeVec<VB>::U U;
	const alpgpu_vector_desc d = c.descs[v];
	DecodeVec<VB>            V;
	V.alp   = d.scheme == ALPGPU_SCHEME_ALP;
	V.bw    = d.bw < 8u * VB ? d.bw : 8u * VB;
	V.cnt   = d.exc_cnt < 1024u ? d.exc_cnt : 1024u; // (zero exactly when the raw count is)
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

// the vector's exception positions into its 16 words of LDS (zeroed, and synchronised on both sides, by exception_mask / exception_masks).
// (`bit` is formed in front of the call, and the two functions below take the workgroup's whole LDS array and index it by the wavefront, because
// that is the form in which the kernels compile to the instruction sequence they had with this code written out in each of them; with the
// shift inside the call, or with a pointer to the wavefront's words, the compiler permutes the loop's instructions: profiles/r17_register_decode.txt.)
template <int VB>
__device__ __forceinline__ void mark_exceptions(const DecodeVec<VB>& V, uint64_t* s_words, uint32_t lane) {
	for (uint32_t j = lane; j < V.cnt; j += 64u) {
		const uint32_t q = V.pos[j];
		if (q < 1024u) {
			const uint32_t bit = 1u << (q & 31u);
			atomicOr(reinterpret_cast<uint32_t*>(s_words) + (q >> 5), bit);
		}
	}
}
// One vector's exception positions as a mask in index order, in the 16 words that the workgroup's LDS array s_exc holds for wavefront `wave`; nothing
// happens for a vector without exceptions (step_request does not read the words then).
template <int VB, int WAVES>
__device__ __forceinline__ void exception_mask(const DecodeVec<VB>& V, uint64_t (&s_exc)[WAVES][16], uint32_t wave, uint32_t lane) {
	if (V.cnt > 0) {
		if (lane < 16u) { s_exc[wave][lane] = 0ull; }
		wave_lds_sync();
		mark_exceptions<VB>(V, s_exc[wave], lane);
		wave_lds_sync();
	}
}
// ... and those of two vectors side by side, s_exc[wave][0] and s_exc[wave][1], under one pair of synchronisations
template <int VB, int WAVES>
__device__ __forceinline__ void exception_masks(const DecodeVec<VB>& A, const DecodeVec<VB>& B, uint64_t (&s_exc)[WAVES][2][16], uint32_t wave, uint32_t lane) {
	if ((A.cnt | B.cnt) > 0) {
		if (lane < 32u) { s_exc[wave][lane >> 4][lane & 15u] = 0ull; }
		wave_lds_sync();
		mark_exceptions<VB>(A, s_exc[wave][0], lane);
		mark_exceptions<VB>(B, s_exc[wave][1], lane);
		wave_lds_sync();
	}
}

// what NB steps of one vector need from memory
template <int VB, uint32_t NB>
struct StepBatch {
	typedef typename DecodeVec<VB>::U U;
	FieldWords<U>        rw[NB];
	FieldWords<uint16_t> lw[NB];
	uint64_t             em[NB]; // wave-uniform: bit l = value 64 m + l is an exception
	U                    ev[NB];
};

// Requests steps b .. b + NB - 1: the packed words, the ALP_RD left words and the exception values by rank; nothing is waited for here.  Every load
// of the batch is requested before the first is used: a step is otherwise its own round trip to memory.  (Both words of a field are always
// loaded, so that no branch stands between the loads: lane_field.hpp.)  The exceptions' values too (ALP: the value's bits; ALP_RD: its left part):
// loaded where they are used, each step with an exception in it would wait for memory once more.  In the generated code that holds for ALP vectors
// only (three or four round trips to memory per vector instead of one per step); for ALP_RD vectors the compiler waits for each exception's left
// part right behind its load, so a step with an exception is a round trip of its own there (profiles/r08_select.txt).  A form that avoids it was
// measured in k_select: every lane loads, without the per-lane branch, one loop per scheme.  It takes 98 registers instead of 81 and cost the
// mixed and float columns more, +4 % and +8 %, than the ALP_RD column gained, -3 %.
// before_exc: the vector's exceptions in the steps done, moved on
template <int VB, uint32_t NB>
__device__ __forceinline__ void step_request(const DecodeVec<VB>& V, const uint64_t* s_words, uint32_t b, uint32_t lane, uint32_t& before_exc, StepBatch<VB, NB>& R) {
	typedef typename DecodeVec<VB>::U U;
	constexpr uint32_t kLanes = VB == 8 ? 16u : 32u; // FastLanes lanes of the value streams
	constexpr uint32_t kLog   = VB == 8 ? 4u : 5u;
#pragma unroll
	for (uint32_t i = 0; i < NB; ++i) {
		R.rw[i] = FieldWords<U> {0, 0};
		R.lw[i] = FieldWords<uint16_t> {0, 0};
		R.em[i] = 0ull;
		R.ev[i] = 0;
	}
	if (V.bw > 0) {
#pragma unroll
		for (uint32_t i = 0; i < NB; ++i) {
			const uint32_t p = 64u * (b + i) + lane;
			R.rw[i]          = load_field_words<U, kLanes>(V.words + (p & (kLanes - 1u)), p >> kLog, V.bw);
		}
	}
	if (!V.alp && V.lbw > 0) {
#pragma unroll
		for (uint32_t i = 0; i < NB; ++i) { R.lw[i] = load_field_words<uint16_t, 64>(V.lefts + lane, b + i, V.lbw); }
	}
	if (V.cnt > 0) {
		uint32_t rank0 = before_exc;
#pragma unroll
		for (uint32_t i = 0; i < NB; ++i) {
			const uint64_t w    = s_words[b + i];
			const uint32_t w_lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(w))); // (the builtin returns int: no sign extension into the high word)
			const uint32_t w_hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(w >> 32)));
			R.em[i]             = (static_cast<uint64_t>(w_hi) << 32) | w_lo;
			const uint32_t rank = rank0 + mbcnt64(R.em[i], 0u);
			if ((R.em[i] >> lane) & 1ull) { R.ev[i] = V.alp ? reinterpret_cast<const U*>(V.rec)[rank] : static_cast<U>(reinterpret_cast<const uint16_t*>(V.rec)[rank]); }
			rank0 += static_cast<uint32_t>(__builtin_popcountll(R.em[i]));
		}
		before_exc = rank0;
	}
}

// The bits of value 64 (b + i) + lane of the vector, what the store decode writes there.  A kernel that stores a value stores these: ALP_RD and
// exception values may be signalling NaNs, and no floating-point operation lies between the streams and the bits.
template <int VB, uint32_t NB>
__device__ __forceinline__ typename DecodeVec<VB>::U step_bits(const DecodeVec<VB>& V, const StepBatch<VB, NB>& R, uint32_t b, uint32_t i, uint32_t lane) {
	typedef typename DecodeVec<VB>::U U;
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
	return bits;
}
// ... as a value of the column's type: a bit cast
template <int VB>
__device__ __forceinline__ typename DecodeVec<VB>::T value_of_bits(typename DecodeVec<VB>::U bits) {
	if constexpr (VB == 8) { return __longlong_as_double(static_cast<long long>(bits)); } else { return __uint_as_float(bits); }
}
template <int VB, uint32_t NB>
__device__ __forceinline__ typename DecodeVec<VB>::T step_value(const DecodeVec<VB>& V, const StepBatch<VB, NB>& R, uint32_t b, uint32_t i, uint32_t lane) {
	return value_of_bits<VB>(step_bits(V, R, b, i, lane));
}

// ---- the glue around the decode ----------------------------------------------------------------------------------------------------------------

// The vector's 128 bytes of bitmap, lane m < 16 holding word m (the other lanes zero); false: no bit is set, the vector's share of the result is
// settled by the caller and nothing of the column is read.
__device__ __forceinline__ bool bitmap_words(const uint64_t* mask, uint64_t v, uint32_t lane, uint64_t& words) {
	words = lane < 16u ? mask[16ull * v + lane] : 0ull;
	return ballot64(words != 0ull) != 0ull;
}

// the share [p_begin, p_end) that the vector beginning at value index r0 has of [first, end): wave-uniform (r0 < end, r0 + 1024 > first)
__device__ __forceinline__ void range_share(uint64_t first, uint64_t end, uint64_t r0, uint32_t& p_begin, uint32_t& p_end) {
	p_begin = first > r0 ? static_cast<uint32_t>(first - r0) : 0u;
	p_end   = end - r0 < 1024u ? static_cast<uint32_t>(end - r0) : 1024u;
}

// (The SET / AND / OR rules of the kernels that write a bitmap, k_select's MASK arm, k_pair's compare arm and k_in_list, are NOT here: they stay
// written out in the three kernels, each with its own `return` or `continue` and its own closing store.  A helper pair was built and timed: behind a
// flag returned in place of the `return`, the launches that settle (nearly) every vector from its 128 bytes of bitmap were 5-6 % slower in k_select
// and k_pair, and even the one-line closing store as a function changes k_pair's and k_in_list's instructions: profiles/r17_register_decode.txt.
// The glue of the persistent kernels that did become functions, and the forms of their calls that kept the kernels' instructions, are in
// persistent_scan.hpp and sorted_list.hpp: profiles/r24_persistent_scan.txt.)

} // namespace alpgpu
