// decode_f32_kernels.hip — fused ALP / ALP_RD column decode for gfx950, single precision.
//
// Replaces, per vector (reference file:line relative to /root/reference):
//   ALP    : generated::falp::fallback::scalar::falp (float)  include/alp/falp.hpp:28-44, src/falp.cpp 32-bit section
//            + alp::decoder<float>::patch_exceptions          include/alp/decoder.hpp:141-149
//   ALP_RD : unffor::unffor (u32 right, u16 left)             include/fastlanes/unffor.hpp:7-15
//            + alp::rd_encoder<float>::decode                 include/alp/rd.hpp:152-178
//
// Same structure as decode_kernels.hip (the measurements that motivate it are listed there): the hardware dispatcher
// hands out small workgroups in vector order; the packed words go HBM -> LDS by LDS-DMA, the exception record becomes
// a 1024-bit mask + staged values, one barrier sits behind the memory latency.  A float vector is 4 KiB of output, so a
// 256-thread workgroup covers one vector with ONE 16-byte store per thread (thread t owns values 4t..4t+3 = one 16-byte
// unit of the FastLanes u32 layout, alp_device_f32.hpp), and V consecutive vectors per workgroup keep the bytes in flight
// per CU at the level of the double-precision kernel (V = 2 moves as many bytes per workgroup as one double vector).
#include "alp_device_f32.hpp"
#include "decode_f32_device.hpp"
#include "decode_policy.hpp"
#include "launch.hpp"
#include "staged_decode.hpp"
#include "wave_minmax.hpp"
#include <cstdlib>

namespace alpgpu {

constexpr int kStageBytesF  = 4480; // >= 31*128 (RD right) + 3*128 (RD left) + 128 pad, and >= 32*128 + 128 (ALP bw 32)
constexpr int kExcStageF    = 256; // exception values (4 bytes; ALP_RD: twice as many 2-byte ones) staged in LDS per vector (round 5, late: 128 -> 256.  bench.py's decimal float column carries 94 exceptions per vector on average, 39 % of its vectors more than 128: decode 0.72-0.73 -> 0.75-0.76; the others unchanged)

struct __attribute__((aligned(16))) DecodeLdsF32 {
	static constexpr bool kPrefixInLds = false; // exception lookup by ds_bpermute
	static constexpr int  kStage       = kStageBytesF;
	static constexpr uint32_t kExcBytes = 4u * kExcStageF;
	uint8_t  stage[kStageBytesF];
	uint32_t mask[32];
	uint8_t  excv[kExcBytes]; // the head of the exception record as it lies in the stream (values first), brought in by LDS-DMA
	uint16_t rdict[8];             // ALP_RD: the rowgroup's dictionary, looked up by ds_read_u16 (round 6: the lookup in registers — a 3-way select through a 64-bit shift — was 13 of the ~27 vector instructions per ALP_RD value)
};

template <bool NT_STORE>
__device__ __forceinline__ void store_quad(float* __restrict__ p, const u32x4& bits) {
	if constexpr (NT_STORE) {
		__builtin_nontemporal_store(bits, reinterpret_cast<u32x4*>(p));
	} else {
		*reinterpret_cast<u32x4*>(p) = bits;
	}
}

// The per-vector constants, read in front of the barrier: ALP_RD = the rowgroup's dictionary (RdDict, alp_device.hpp); ALP vectors use
// the same two words for lo = FACT_ARR[f], hi = bits of FRAC_ARR[e]
__device__ __forceinline__ RdDict load_vector_consts_f32(const alpgpu_rowgroup_state* __restrict__ rgs, uint64_t v, const alpgpu_vector_desc& d) {
	if (d.scheme != ALPGPU_SCHEME_ALP) { return load_rd_dict(rgs, v, true); } // wave-uniform
	return RdDict {static_cast<uint64_t>(kFactArrF[d.f]), static_cast<uint64_t>(__float_as_uint(kFracArrF[d.e]))};
}

// one quad, after its words have arrived: thread tid (of 256: wavefront `wave`, lane) owns values 4*tid .. 4*tid+3; `em` = the vector's
// exception mask as this wavefront sees it (ignored when the vector has none), L = where staged exception values live.
// SINK (as in decode_kernels.hip) = kSinkStoreF: the quad is stored.  kSinkSumF: its four values are widened to double
// (exact) and added to `acc` in index order.  kSinkCountF: `acc` counts the values v with lo <= v <= hi (NaN never does).
constexpr int kSinkStoreF = 0, kSinkSumF = 1, kSinkCountF = 2;
// kSinkMinMaxF (alpgpu_zone_map_f32): mm[0] / mm[1] = the smallest / largest value that is not a NaN (wave_minmax.hpp: minmax_take); `acc` is unused.
constexpr int kSinkMinMaxF = 3;
// HBM_EXC = false: the caller knows (wave-uniform) that every exception value of the vector is in the LDS stage — this instance has no load from HBM in it, so
// the compiler puts no s_waitcnt vmcnt(0) in front of the quad's store (stores count in vmcnt on gfx9: with the rare load in the code, every store of a
// wavefront waited for the one before it — decode_kernels.hip cured the double kernel of this in round 5, the float kernel followed late in the round).
template <bool NT_STORE, int SINK, class LDS, bool HBM_EXC = true>
__device__ __forceinline__ void finish_quad_f32(const LDS& L, const QuadWords& w, const alpgpu_vector_desc& d, const RdDict& dict, const ExcMask& em,
                                                const uint8_t* __restrict__ rec, float* __restrict__ dst, int tid, int wave, int lane, double* acc,
                                                float range_lo, float range_hi, float* mm = nullptr) {
	const int bw   = d.bw;
	const int cnt  = d.exc_cnt;
	const int a    = tid & 7;
	const int row  = tid >> 3;
	uint32_t  hits = 0;
	int       rank = 0;
	const bool all_staged = !HBM_EXC || cnt <= (d.scheme == ALPGPU_SCHEME_ALP ? kExcStageF : 2 * kExcStageF); // wave-uniform: every exception value of the vector is in the LDS stage
	// Round 6: the SINKS skip an ALP vector's exception positions here (the position counts as +0.0 / as outside the range) and take the exception VALUES in one
	// pass behind the quads (sink_exception_values_f32) — the per-value lookup (rank, four divergent blocks per quad, an LDS read and its wait each) was ~170 of
	// the ~540 vector instructions per vector of an exception-heavy column (profiles/r05_float_sink.txt); include/alpgpu.h documents the order.  ALP_RD vectors
	// (few exceptions, and an exception there is a LEFT part that needs its position's right part) keep the lookup in place.
	constexpr bool kApart = SINK != kSinkStoreF;
	if (kApart && cnt > 0 && d.scheme == ALPGPU_SCHEME_ALP) {
		const int wi = 8 * wave + (lane >> 3);
		uint32_t  word;
		if constexpr (LDS::kPrefixInLds) {
			word = L.mask[wi];
		} else {
			word = static_cast<uint32_t>(__shfl(static_cast<int>(em.word), wi));
		}
		hits = (word >> (4 * a)) & 0xFu;
	} else if (cnt > 0) { // the quad's four mask bits and the rank of its first exception
		const int wi = 8 * wave + (lane >> 3);
		uint32_t  word;
		int       pref;
		if constexpr (LDS::kPrefixInLds) { // k_sink_direct_f32: out of the wavefront's LDS, not by ds_bpermute while its loads are in flight (staged_decode.hpp: exception_hits_lds)
			word = L.mask[wi];
			pref = static_cast<int>(L.pref[wi]);
		} else {
			word = static_cast<uint32_t>(__shfl(static_cast<int>(em.word), wi));
			pref = __shfl(em.excl, wi);
		}
		const int      b0   = 4 * a;
		hits                = (word >> b0) & 0xFu;
		rank                = pref + __builtin_popcount(word & ((1u << b0) - 1u));
	}
	// FastLanes u32 unpack (alp_device_f32.hpp: unpack_quad_u32): (w1 << (32 - s)) without the undefined shift by 32 when s == 0
	// ... which is the 64-bit funnel {w1, w0} >> s: ONE v_alignbit_b32 per value (it takes the amount modulo 32, so s = 0 yields w0), where the
	// spelled-out form cost four (round 4: the one-wavefront sink is bound by its vector instructions — 489 per vector before this)
	const uint32_t s    = static_cast<uint32_t>(row * bw) & 31u;
	const uint32_t msk  = bw_mask32(bw);
	u32x4          q;
#pragma unroll
	for (int c = 0; c < 4; ++c) { q[c] = __builtin_amdgcn_alignbit(w.w1[c], w.w0[c], s) & msk; }
	u32x4          out;
	if (d.scheme == ALPGPU_SCHEME_ALP) {
		const uint32_t base = static_cast<uint32_t>(d.base);
		const uint32_t fact = static_cast<uint32_t>(dict.lo);
		const float    frac = __uint_as_float(static_cast<uint32_t>(dict.hi));
		// Conversion shortcut, decided once per vector from its descriptor (wave-uniform, scalar arithmetic; the double kernels' kDecodeTab idea):
		// if every integer base + digit of the vector lies in [-2^24, 2^24] and times 10^f stays inside int32, then (float)(int32)(value * 10^f)
		// — a quarter-rate 32-bit integer multiply and a conversion — is the correctly rounded product of two exactly representable floats, i.e.
		// the IEEE product (float)value * 10^f (10^f = 2^f 5^f with 5^10 < 2^24: exact for every f <= 10): same bits, one full-rate multiply.
		// (the bound from a table — round 5: as a division it was ~25 scalar and vector instructions, and the one-wavefront sink, which runs this
		//  function four times per vector and is bound by its instruction issue, did it four times)
		const int64_t lo64 = static_cast<int64_t>(static_cast<int32_t>(base)), hi64 = lo64 + static_cast<int64_t>(bw_mask32(bw));
		const int64_t bnd  = static_cast<int64_t>(kShortcutBoundF[d.f]); // min(2^24, (2^31 - 1) / 10^f) for f <= 9; 0 for f = 10 (10^10 does not fit: literal path)
		const bool    shortcut = bw <= 24 && lo64 >= -bnd && hi64 <= bnd;
		if (shortcut) {
			const float fact_f = static_cast<float>(fact);
#pragma unroll
			for (int c = 0; c < 4; ++c) { out[c] = __float_as_uint((static_cast<float>(static_cast<int32_t>(q[c] + base)) * fact_f) * frac); }
		} else {
#pragma unroll
			for (int c = 0; c < 4; ++c) { out[c] = __float_as_uint(decode_value_f32(static_cast<int32_t>(q[c] + base), fact, frac)); }
		}
		if constexpr (kApart) {
			// (the sinks: an exception position contributes +0.0f — (double)(+0.0f) added to a partial that is never -0.0 leaves it as it is — or, for COUNT and MIN / MAX, a NaN)
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				if (hits & (1u << c)) { out[c] = SINK == kSinkSumF ? 0u : 0x7FC00000u; }
			}
		} else if (hits) { // (a branch-free form — every lane reads the staged value it WOULD take, then selects — was measured in round 5: no difference, 64 VGPRs; profiles/r05_float_sink.txt)
#pragma unroll
			for (int c = 0; c < 4; ++c) {
				if (hits & (1u << c)) {
					out[c] = fetch_exception<4>(L, rec, rank, all_staged);
					++rank;
				}
			}
		}
	} else {
		// ALP_RD: right parts = u32 lanes (bw = rbw, base 0); left parts = u16 lanes, 64 streams x 16 rows (value i ->
		// lane64 = i & 63, row = i >> 6, word k at left[64*k + lane64]): the quad shares row tid >> 4 and is the aligned
		// 8-byte group (tid & 15) of every left word row.
		const int      rbw  = bw;
		const int      lbw  = d.lbw;
		const uint32_t lmsk = (1u << lbw) - 1u;
		const uint64_t dlo = dict.lo, dhi = dict.hi;
		(void)dlo, (void)dhi;
		const int      ls   = ((tid >> 4) * lbw) & 15;
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			const uint32_t f0  = static_cast<uint32_t>(w.l0 >> (16 * c)) & 0xFFFFu;
			const uint32_t f1  = static_cast<uint32_t>(w.l1 >> (16 * c)) & 0xFFFFu;
			const uint32_t idx = ((f0 >> ls) | (f1 << (16 - ls))) & lmsk;
			uint32_t       l   = L.rdict[idx & 7u];
			if (hits & (1u << c)) {
				l = fetch_exception<2>(L, rec, rank, all_staged);
				++rank;
			}
			out[c] = (l << rbw) | q[c];
		}
	}
	if constexpr (SINK == kSinkSumF) {
#pragma unroll
		for (int c = 0; c < 4; ++c) { *acc += static_cast<double>(__uint_as_float(out[c])); }
	} else if constexpr (SINK == kSinkCountF) {
#pragma unroll
		for (int c = 0; c < 4; ++c) {
			const float v = __uint_as_float(out[c]);
			*acc += (v >= range_lo && v <= range_hi) ? 1.0 : 0.0;
		}
	} else if constexpr (SINK == kSinkMinMaxF) {
#pragma unroll
		for (int c = 0; c < 4; ++c) { minmax_take(mm[0], mm[1], __uint_as_float(out[c])); }
	} else {
		store_quad<NT_STORE>(dst + 4 * tid, out);
		// (the two instances' stores must stay two stores: merged into one behind the join of their callers' branch, the wait for the rare load is back in front of it)
		if constexpr (HBM_EXC) {
			asm volatile("; quad stored (exception values beyond the stage possible)" ::: "memory");
		} else {
			asm volatile("; quad stored (exception values all staged)" ::: "memory");
		}
	}
}

// the sinks' second pass over an ALP vector with exceptions: lane L takes the values j = L, L + 64, ... in ascending order (staged ones from LDS, the rest from
// the stream) and adds them to `total` (SUM: widened; COUNT: those inside [lo, hi])
template <int SINK, class LDS>
__device__ __forceinline__ void sink_exception_values_f32(const LDS& L, const uint8_t* __restrict__ rec, int cnt, int lane, double& total, float range_lo, float range_hi) {
	for (int j = lane; j < cnt; j += 64) {
		uint32_t bits;
		if (j < kExcStageF) {
			bits = reinterpret_cast<const uint32_t*>(L.excv)[j];
		} else {
			bits = reinterpret_cast<const uint32_t*>(rec)[j];
		}
		const float v = __uint_as_float(bits);
		if constexpr (SINK == kSinkCountF) {
			total += (v >= range_lo && v <= range_hi) ? 1.0 : 0.0;
		} else {
			total += static_cast<double>(v);
		}
	}
}

// ... the same pass for MIN / MAX: an exception value that is a NaN is dropped like any other NaN of the vector
template <class LDS>
__device__ __forceinline__ void minmax_exception_values_f32(const LDS& L, const uint8_t* __restrict__ rec, int cnt, int lane, float& mn, float& mx) {
	for (int j = lane; j < cnt; j += 64) {
		uint32_t bits;
		if (j < kExcStageF) {
			bits = reinterpret_cast<const uint32_t*>(L.excv)[j];
		} else {
			bits = reinterpret_cast<const uint32_t*>(rec)[j];
		}
		minmax_take(mn, mx, __uint_as_float(bits));
	}
}

// one vector of a staged workgroup, after its packed words / exception mask are visible in L
template <bool NT_STORE, int SINK = kSinkStoreF>
__device__ __forceinline__ void decode_staged_vector_f32(const DecodeLdsF32& L, const alpgpu_vector_desc& d, const RdDict& dict,
                                                         const uint8_t* __restrict__ rec, float* __restrict__ dst, int tid, int wave, int lane,
                                                         double* acc = nullptr, float range_lo = 0.0f, float range_hi = 0.0f) {
	ExcMask em {0u, 0};
	if (d.exc_cnt > 0) { em = load_exception_mask(L, lane); }
	const QuadWords w = request_quad_f32(StagedWordsF {L.stage}, d, tid);
	if (SINK == kSinkStoreF && d.exc_cnt <= (d.scheme == ALPGPU_SCHEME_ALP ? kExcStageF : 2 * kExcStageF)) { // workgroup-uniform
		finish_quad_f32<NT_STORE, SINK, DecodeLdsF32, false>(L, w, d, dict, em, rec, dst, tid, wave, lane, acc, range_lo, range_hi);
	} else {
		finish_quad_f32<NT_STORE, SINK, DecodeLdsF32, true>(L, w, d, dict, em, rec, dst, tid, wave, lane, acc, range_lo, range_hi);
	}
}

// SINK != kSinkStoreF: `out` is the per-vector result array instead (double sums / uint32 counts)
template <int V, bool NT_STORE, int SINK = kSinkStoreF>
__global__ __launch_bounds__(kDecThreads) void k_decode_column_f32(const alpgpu_vector_desc* __restrict__ descs,
                                                                    const alpgpu_rowgroup_state* __restrict__ rgs, const uint8_t* __restrict__ packed,
                                                                    const uint8_t* __restrict__ excs, float* __restrict__ out, uint64_t n_vectors,
                                                                    uint64_t wg_offset, float range_lo, float range_hi, uint64_t* __restrict__ progress, uint64_t progress_tag,
                                                                    uint32_t gate) {
	__shared__ DecodeLdsF32 L[V];
	const int      tid  = static_cast<int>(threadIdx.x);
	const int      lane = tid & 63;
	const int      wave = wave_in_wg();
	const uint64_t v0   = (wg_offset + blockIdx.x) * V;
	if (v0 >= n_vectors) { return; }
	if constexpr (SINK == kSinkStoreF) {
		// a candidate launch of an unhinted decode runs only if the plan says so; the read-ahead's pace: every 128th workgroup says where the launch is
		// (decode_kernels.hip: k_decode_column; round 6: the float store decode reports too)
		if (gate != 0u && progress[kCtxWordShape] != static_cast<uint64_t>(gate)) { return; } // (kernel argument: uniform)
		if (progress != nullptr && (blockIdx.x & 127u) == 0 && tid == 0) { __hip_atomic_store(progress, progress_tag | v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
	}

	alpgpu_vector_desc d[V];
	RdDict             dict[V];
	stage_vectors<4>(L, d, dict, descs, packed, excs, v0, n_vectors, tid, wave, [&](uint64_t v, const alpgpu_vector_desc& dv) { return load_vector_consts_f32(rgs, v, dv); });
	if constexpr (SINK != kSinkStoreF) {
		// per-vector result: thread partial over its quad (index order, in double), then staged_decode.hpp: finish_vector_sinks
		double acc[V];
#pragma unroll
		for (int i = 0; i < V; ++i) {
			acc[i] = 0.0;
			if (v0 + i < n_vectors) {
				decode_staged_vector_f32<NT_STORE, SINK>(L[i], d[i], dict[i], excs + d[i].exc_off, nullptr, tid, wave, lane, &acc[i], range_lo,
				                                         range_hi);
			}
		}
		finish_vector_sinks<SINK == kSinkCountF>(L, acc, reinterpret_cast<double*>(out), v0, n_vectors, wave, lane, [&](int i, double& total) {
			if (d[i].exc_cnt > 0 && d[i].scheme == ALPGPU_SCHEME_ALP) { sink_exception_values_f32<SINK>(L[i], excs + d[i].exc_off, d[i].exc_cnt, lane, total, range_lo, range_hi); }
		});
		return;
	}
#pragma unroll
	for (int i = 0; i < V; ++i) {
		if (v0 + i < n_vectors) {
			decode_staged_vector_f32<NT_STORE>(L[i], d[i], dict[i], excs + d[i].exc_off, out + (v0 + i) * kVec, tid, wave, lane);
		}
	}
}

static unsigned pad_bytes(int pad_kib) { return pad_kib > 0 ? static_cast<unsigned>(pad_kib) * 1024u : 0u; } // unused dynamic LDS that caps the workgroups resident per CU, as the double decode does by width

template <int V>
static int launch_v(hipStream_t stream, const alpgpu_column* col, float* d_out, const DecodeShape& shape, uint64_t* progress, uint64_t tag, uint32_t gate) {
	if (gate != 0 && progress == nullptr) { gate = 0; }
	const auto kernel = shape.plain_stores ? k_decode_column_f32<V, false> : k_decode_column_f32<V, true>;
	return launch_over_column(kernel, wgs_of(col, V), dec_block(), pad_bytes(shape.pad_kib), stream, col, d_out, 0.0f, 0.0f, progress, tag, gate);
}

static int launch_store_direct_f32(hipStream_t stream, const alpgpu_column* col, float* d_out, int pad_kib, uint64_t* progress, uint64_t progress_tag); // (below, behind its kernel)
int launch_decode_column_f32(hipStream_t stream, const alpgpu_column* col, float* d_out, const DecodeShape& shape, uint64_t* progress, uint64_t progress_tag, uint32_t gate) {
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	if (shape.family == kDecodeWaveDirect) { return launch_store_direct_f32(stream, col, d_out, shape.pad_kib, progress, progress_tag); } // (no gate: never a candidate of an unhinted decode)
	switch (shape.vectors_per_wg) {
	case 1: return launch_v<1>(stream, col, d_out, shape, progress, progress_tag, gate);
	case 2: return launch_v<2>(stream, col, d_out, shape, progress, progress_tag, gate);
	default: return launch_v<4>(stream, col, d_out, shape, progress, progress_tag, gate);
	}
}

template <int SINK, int V>
static int launch_sink_f32(hipStream_t stream, const alpgpu_column* col, void* d_result, float lo, float hi) {
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	return launch_over_column(k_decode_column_f32<V, false, SINK>, wgs_of(col, V), dec_block(), 0, stream, col, static_cast<float*>(d_result), lo, hi, kNoProgress, 0ull, 0u);
}

// ---- the float sinks with ONE wavefront per vector, packed words straight from HBM (decode_kernels.hip: k_sink_direct) ----------------
// Lane L does what threads L, 64 + L, 128 + L, 192 + L of the staged kernel do: four quads, their partials kept apart (p[w][L]), all four
// quads' words requested before the first is used; then (p0 + p1) + (p2 + p3) and the adjacent-lane tree: the same bits.
constexpr int kSinkStageF32 = 3584; // bytes of packed words (bit widths <= 28) a wavefront of k_sink_direct_f32 stages in its LDS by LDS-DMA (0: none)
constexpr int kSinkStageF32MaxExc = 1024; // ... only for vectors with at most this many exceptions (round 6: any — it was 48 while the exception values were looked up per quad; with them taken behind the quads the stage pays at every count: +1.5 %, call 26)
struct __attribute__((aligned(16))) SinkWaveLdsF32 {
	static constexpr bool kPrefixInLds = true;
	static constexpr uint32_t kExcBytes = 4u * kExcStageF;
	uint8_t  stage[kSinkStageF32 + 128]; // + the unit row past the end that the unpack reads and masks off
	uint32_t mask[32];
	uint8_t  excv[kExcBytes];
	uint32_t pref[32]; // exceptions in front of mask word i
	uint16_t rdict[8]; // ALP_RD: the rowgroup's dictionary (DecodeLdsF32)
};
template <int SINK>
__global__ __launch_bounds__(kDecThreads, 8) void k_sink_direct_f32(const alpgpu_vector_desc* __restrict__ descs, const alpgpu_rowgroup_state* __restrict__ rgs,
                                                                      const uint8_t* __restrict__ packed, const uint8_t* __restrict__ excs, double* __restrict__ out,
                                                                      uint64_t n_vectors, uint64_t wg_offset, float lo, float hi, uint64_t* __restrict__ progress, uint64_t progress_tag) {
	#ifdef ALPGPU_SINK_REGISTER_MARGIN
	asm volatile("" ::: "v64"); // decode_kernels.hip: k_sink_direct
#endif
	__shared__ SinkWaveLdsF32 S[kDecWaves];
	const int      lane = static_cast<int>(threadIdx.x) & 63;
	const int      wv   = wave_in_wg();
	const uint64_t v    = (wg_offset + blockIdx.x) * kDecWaves + wv;
	if (v >= n_vectors) { return; } // wave-uniform; no barrier anywhere in this kernel
	if constexpr (SINK == kSinkStoreF) { // the store form reports where the launch is, for the read-ahead (k_decode_column_f32 does the same): every 32nd workgroup = every 128th vector
		if (progress != nullptr && (blockIdx.x & 31u) == 0 && threadIdx.x == 0) { __hip_atomic_store(progress, progress_tag | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
	}
	SinkWaveLdsF32&          L      = S[wv];
	const alpgpu_vector_desc d      = descs[v];
	const RdDict             dict   = load_vector_consts_f32(rgs, v, d);
	const uint8_t*           rec    = excs + d.exc_off;
	const bool               is_alp = d.scheme == ALPGPU_SCHEME_ALP;
	const int                cnt    = d.exc_cnt;
	// staged (round 4; the double sink had it first — VERDICT round 3, item 6: "is the stage arm even taken for float?" — there was none): either scheme — ALP_RD
	// vectors right words, then left words, as they lie in the stream (late round 4) — and any exception count
	const int     stage_words = static_cast<int>(d.bw) + (is_alp ? 0 : static_cast<int>(d.lbw));
	const bool    staged = 128 * stage_words <= kSinkStageF32 && cnt <= kSinkStageF32MaxExc; // wave-uniform
	const ExcMask em     = stage_wave_vector<4>(L, d, packed, rec, staged, lane);
	const BufferWordsF words = packed_word_resources<BufferWordsF>(packed + d.packed_off, d.bw, d.lbw, is_alp);
	if (!is_alp) { // wave-uniform: the dictionary into the wavefront's LDS, behind the issue of every load (its own scalar loads are waited for here, not in front of them)
		if (lane < 4) { stage_rd_dictionary(L, dict, lane); }
		wave_lds_sync();
	}
	QuadWords w[4];
	if (staged) {
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // LDS-DMA completion is not tracked through the LDS for the compiler
		wave_lds_sync();
		const StagedWordsF sw {L.stage};
#pragma unroll
		for (int q = 0; q < 4; ++q) { w[q] = request_quad_f32(sw, d, 64 * q + lane); }
	} else
	{
#pragma unroll
		for (int q = 0; q < 4; ++q) { w[q] = request_quad_f32(words, d, 64 * q + lane); }
	}
	if constexpr (SINK == kSinkStoreF) {
		// Round 6: the same wavefront as a STORE decoder (ALPGPU_OPT_DECODE_VECTORS_PER_WG = 8 for float columns): lane L's four quads are the 16-byte units L, 64 + L,
		// 128 + L, 192 + L of the vector — four store instructions of 1 KiB each, no barrier, one wave-uniform prologue per vector instead of four.
		float* dst = reinterpret_cast<float*>(out) + v * kVec;
		if (cnt <= (is_alp ? kExcStageF : 2 * kExcStageF)) { // wave-uniform: every exception value is staged — the instance without a load between the stores
#pragma unroll
			for (int q = 0; q < 4; ++q) { finish_quad_f32<true, kSinkStoreF, SinkWaveLdsF32, false>(L, w[q], d, dict, em, rec, dst, 64 * q + lane, q, lane, nullptr, 0.0f, 0.0f); }
		} else {
#pragma unroll
			for (int q = 0; q < 4; ++q) { finish_quad_f32<true, kSinkStoreF, SinkWaveLdsF32, true>(L, w[q], d, dict, em, rec, dst, 64 * q + lane, q, lane, nullptr, 0.0f, 0.0f); }
		}
		return;
	}
	if constexpr (SINK == kSinkMinMaxF) { // the record {min, max}: the quads, then an ALP vector's exception values, then the wavefront; one 8-byte store per vector
		float mm[2] = {__builtin_inff(), -__builtin_inff()};
#pragma unroll
		for (int q = 0; q < 4; ++q) { finish_quad_f32<false, SINK>(L, w[q], d, dict, em, rec, nullptr, 64 * q + lane, q, lane, nullptr, 0.0f, 0.0f, mm); }
		if (is_alp && cnt > 0) { minmax_exception_values_f32(L, rec, cnt, lane, mm[0], mm[1]); }
		wave_minmax_f32(mm[0], mm[1]);
		if (lane == 0) { reinterpret_cast<float2*>(out)[v] = make_float2(mm[0], mm[1]); }
		return;
	}
	double part[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
	for (int q = 0; q < 4; ++q) { finish_quad_f32<false, SINK>(L, w[q], d, dict, em, rec, nullptr, 64 * q + lane, q, lane, &part[q], lo, hi); }
	double total = (part[0] + part[1]) + (part[2] + part[3]);
	if (is_alp && cnt > 0) { sink_exception_values_f32<SINK>(L, rec, cnt, lane, total, lo, hi); }
	store_vector_result<SINK == kSinkCountF>(out, v, total, lane);
}

// one wavefront per vector, four vectors per workgroup, no barrier: k_sink_direct_f32 as a store decoder (non-temporal stores)
static int launch_store_direct_f32(hipStream_t stream, const alpgpu_column* col, float* d_out, int pad_kib, uint64_t* progress, uint64_t progress_tag) {
	return launch_over_column(k_sink_direct_f32<kSinkStoreF>, wgs_of(col, kDecWaves), dec_block(), pad_bytes(pad_kib), stream, col, reinterpret_cast<double*>(d_out), 0.0f, 0.0f, progress, progress_tag);
}

int launch_sink_direct_f32(hipStream_t stream, const alpgpu_column* col, float lo, float hi, void* d_out, bool count) {
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	double* out = static_cast<double*>(d_out);
	if (count) { return launch_over_column(k_sink_direct_f32<kSinkCountF>, wgs_of(col, kDecWaves), dec_block(), 0, stream, col, out, lo, hi, kNoProgress, 0ull); }
	return launch_over_column(k_sink_direct_f32<kSinkSumF>, wgs_of(col, kDecWaves), dec_block(), 0, stream, col, out, 0.0f, 0.0f, kNoProgress, 0ull);
}

// d_zones[v] = {min, max} of vector v's decoded values, NaNs ignored (include/alpgpu.h: zone maps); n_vectors > 0
int launch_zone_map_f32(hipStream_t stream, const alpgpu_column* col, void* d_zones) {
	return launch_over_column(k_sink_direct_f32<kSinkMinMaxF>, wgs_of(col, kDecWaves), dec_block(), 0, stream, col, static_cast<double*>(d_zones), 0.0f, 0.0f, kNoProgress, 0ull);
}

// two vectors per workgroup: measured 1.57 / 1.30 / 1.37 ms per 1 Mi vectors for 1 / 2 / 4
int launch_decode_sum_f32(hipStream_t stream, const alpgpu_column* col, double* d_sums) { return launch_sink_f32<kSinkSumF, 2>(stream, col, d_sums, 0.0f, 0.0f); }

int launch_decode_count_range_f32(hipStream_t stream, const alpgpu_column* col, float lo, float hi, uint32_t* d_counts) {
	return launch_sink_f32<kSinkCountF, 2>(stream, col, d_counts, lo, hi);
}

} // namespace alpgpu
