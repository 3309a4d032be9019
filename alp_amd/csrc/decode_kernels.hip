// decode_kernels.hip — fused ALP / ALP_RD column decode for gfx950.
//
// Replaces, per vector (reference file:line relative to /root/reference):
//   ALP    : generated::falp::fallback::scalar::falp   include/alp/falp.hpp:10-26, src/falp.cpp:42440 (:114-121 per value)
//            + alp::decoder<double>::patch_exceptions   include/alp/decoder.hpp:141-149
//   ALP_RD : unffor::unffor (u64 right, u16 left)       src/fastlanes_generated_unffor.cpp:23010, :22846
//            + alp::rd_encoder<double>::decode          include/alp/rd.hpp:152-178
//
// Launch shape (measured: profiles/r01_membw_store_structure.txt, r01_membw2_waves_per_vector.txt,
// r01_decode_ablation.txt): the HBM subsystem of MI355X sustains ~5.2-5.4 TB/s of mixed read+write traffic from a
// persistent grid-stride kernel in which every wavefront streams its own 8 KiB vector (and the arithmetic is NOT
// the limiter there: dropping it changes nothing), but ~6.0-6.3 TB/s when the hardware dispatcher hands out ONE
// SMALL WORKGROUP PER VECTOR in order — the in-flight footprint stays compact and in address order.  So:
// grid = n_vectors, one 256-thread workgroup (4 wavefronts) per 1024-value vector, wavefront q owns steps
// m = 2q, 2q+1 (a contiguous 2 KiB quarter of the output):
//   1. one 32-byte descriptor load (wave-uniform scalar load),
//   2. the vector's packed words (128*bw bytes) go HBM -> LDS once, 16 bytes per thread per load,
//   3. the exception record (if any) becomes a 1024-bit position mask in LDS (+ values staged in LDS); every
//      wavefront keeps the 32-word exclusive prefix of the mask's popcounts in registers,
//   4. each lane unpacks its value pairs, applies base/FACT/FRAC (or the RD dictionary glue), substitutes
//      exceptions by rank, and stores 16 bytes -> every store instruction writes 1 KiB contiguous.
// What bounds it now (profiles/r01_time_waves.txt, r01_time_prefetch.txt, r01_time_v2.txt): a workgroup lives for two
// dependent HBM round trips (descriptor, then packed words) and 8 workgroups fit per CU (32-wave cap), i.e.
// ~2 vectors/us/CU regardless of bit width.  Keeping more vectors in flight (2 waves per vector, or 2 vectors per
// workgroup = ALPGPU_OPT_DECODE_VECTORS_PER_WG 2) lifts narrow widths (bw 4: 4.1 -> 5.2 TB/s, bw 16: 5.6 -> 6.1) but
// the larger in-flight window costs 5-8 % on wide widths and on the mixed-width benchmark column (0.72 vs 0.79 of
// peak); an L2 prefetch of the descriptor 2-16 Ki vectors ahead did not move anything.  Default: 1 vector, 4 waves.
// HBM traffic per vector is the algorithmic minimum: 32 B descriptor + 128*bw B packed + exception record read,
// 8192 B written (rocprofv3 FETCH_SIZE/WRITE_SIZE: profiles/*_pmc.json); no intermediate goes to HBM.
#include "alp_device.hpp"
#include "decode_policy.hpp"
#include "launch.hpp"
#include "staged_decode.hpp"
#include "wave_minmax.hpp"
#include <cstdlib>

namespace alpgpu {

constexpr int kStepsPerWave = 8 / kDecWaves;
constexpr int kDecodeBatch  = 4; // steps whose words are requested together (decode_vector_quarters)
constexpr int kStageBytes   = 8704; // >= 63*128 (RD right) + 3*128 (RD left) + 128 pad, and >= 64*128 + 128 (ALP bw 64)
constexpr int kExcStage     = 128; // 8-byte exception values staged in LDS per vector (four times as many 2-byte ALP_RD ones); the rest are read from HBM on use
constexpr uint32_t kExcStageBytes = 8u * kExcStage;

template <int STAGE, int EXC = kExcStage>
struct __attribute__((aligned(16))) DecodeLdsT {
	static constexpr bool kPrefixInLds = false; // exception lookup by ds_bpermute (exception_hits)
	static constexpr int  kStage       = STAGE;
	static constexpr uint32_t kExcBytes = 8u * EXC;
	uint8_t  stage[STAGE];
	uint32_t mask[32];
	uint8_t  excv[kExcBytes]; // the head of the exception record as it lies in the stream (its values come first), brought in by LDS-DMA
	uint16_t rdict[8];        // ALP_RD: the rowgroup's dictionary, looked up by ds_read_u16 (round 6; decode_f32_kernels.hip: DecodeLdsF32)
};
using DecodeLds = DecodeLdsT<kStageBytes>;
// Round 6: columns whose vectors carry MORE exceptions than the 128-entry stage holds on average (bench.py's 10 %-exceptions column: 187 per vector) decode every
// value beyond the stage with a load from HBM in the unpack loop (the run-time form of decode_vector_quarters).  A 256-entry stage lifts that column from 0.72 to 0.77
// of the HBM peak — and costs every OTHER column 2-6 % (1 KiB more LDS per vector: city_temperature 0.78 -> 0.74, nyc29 0.81 -> 0.78; call 6), so it is an instance
// of its own, launched for columns whose hints say so (decode_policy.hpp: policy_shape_f64, DecodeShape::many_exc).
using DecodeLdsManyExc = DecodeLdsT<kStageBytes, 2 * kExcStage>;

template <bool NT_STORE>
__device__ __forceinline__ void store_pair(double2* __restrict__ p, double x, double y) {
	typedef double d2v __attribute__((ext_vector_type(2)));
	d2v o;
	o.x = x;
	o.y = y;
	if constexpr (NT_STORE) {
		__builtin_nontemporal_store(o, reinterpret_cast<d2v*>(p));
	} else {
		*reinterpret_cast<d2v*>(p) = o;
	}
}

// ---- one vector, after its packed words / exception mask are visible in L --------------------------------------
// SINK = kSinkStore: the decoded pair is stored (dst).  kSinkSum: it is added to `acc` instead, x then y, in step order —
// the fixed order tests/test_decode_sum_gpu.py reproduces on the host (decode fused into its
// consumer, the shape of publication/source_code/bench_end_to_end/src/benchmarks/alp/queries/q1.cpp:63-104, without the
// 8 KiB per vector of decoded doubles ever reaching HBM).
// kSinkCount: `acc` counts the values v with lo <= v <= hi (a predicate pushed into the decode; NaN never qualifies).
constexpr int kSinkStore = 0, kSinkSum = 1, kSinkCount = 2;
// kSinkProbe (alpgpu_debug_decode_probe): the consumers' memory traffic and latency chain without the unpack — descriptors, packed
// words into LDS, exceptions, the barrier — every thread then just adds up the staged 16-byte units it would have unpacked.
constexpr int kSinkProbe = 3;
// kSinkMinMax (alpgpu_zone_map_f64): acc[0] / acc[1] = the smallest / largest value that is not a NaN (wave_minmax.hpp: minmax_take).  Minimum and
// maximum do not depend on the order, so every quarter of a vector goes into the same pair (sink_acc).
constexpr int kSinkMinMax = 4;
template <int SINK>
__device__ __forceinline__ double* sink_acc(double* acc, int quarter) {
	return SINK == kSinkMinMax ? acc : acc + quarter;
}
template <int SINK>
__device__ __forceinline__ void consume_pair(double ox, double oy, double* acc, double lo, double hi) {
	if constexpr (SINK == kSinkSum) {
		*acc += ox;
		*acc += oy;
	} else if constexpr (SINK == kSinkMinMax) {
		minmax_take(acc[0], acc[1], ox);
		minmax_take(acc[0], acc[1], oy);
	} else {
		*acc += (ox >= lo && ox <= hi) ? 1.0 : 0.0; // small integers: exact in double
		*acc += (oy >= lo && oy <= hi) ? 1.0 : 0.0;
	}
}

// One table for everything the ALP decode reads by descriptor: entry i = {FACT_ARR[i], 10^i as a double, the conversion shortcut's bound for
// f = i, FRAC_ARR[i]} — one address computation on the scalar unit instead of four (the decode kernels run eight wavefronts per SIMD, each
// repeating the same wave-uniform prologue, and the scalar unit is what saturates first: profiles/r03_consumers.txt).  The bound is
// min(2^51 - 1, floor((2^63 - 1) / 10^i)): the largest |integer| that is exact as a double in the shortcut's range AND whose product with
// 10^i stays inside int64.  Literals as in alp_device.hpp (constants.hpp:66-154).
struct DecodeTabEntry {
	int64_t  fact;
	double   fact_d;
	uint64_t shortcut_bound;
	double   frac;
};
__device__ __constant__ const DecodeTabEntry kDecodeTab[21] = {
    {1ll, 1.0, 2251799813685247ull, 1.0},
    {10ll, 10.0, 2251799813685247ull, 0.1},
    {100ll, 100.0, 2251799813685247ull, 0.01},
    {1000ll, 1000.0, 2251799813685247ull, 0.001},
    {10000ll, 10000.0, 922337203685477ull, 0.0001},
    {100000ll, 100000.0, 92233720368547ull, 0.00001},
    {1000000ll, 1000000.0, 9223372036854ull, 0.000001},
    {10000000ll, 10000000.0, 922337203685ull, 0.0000001},
    {100000000ll, 100000000.0, 92233720368ull, 0.00000001},
    {1000000000ll, 1000000000.0, 9223372036ull, 0.000000001},
    {10000000000ll, 10000000000.0, 922337203ull, 0.0000000001},
    {100000000000ll, 100000000000.0, 92233720ull, 0.00000000001},
    {1000000000000ll, 1000000000000.0, 9223372ull, 0.000000000001},
    {10000000000000ll, 10000000000000.0, 922337ull, 0.0000000000001},
    {100000000000000ll, 100000000000000.0, 92233ull, 0.00000000000001},
    {1000000000000000ll, 1000000000000000.0, 9223ull, 0.000000000000001},
    {10000000000000000ll, 10000000000000000.0, 922ull, 0.0000000000000001},
    {100000000000000000ll, 100000000000000000.0, 92ull, 0.00000000000000001},
    {1000000000000000000ll, 1000000000000000000.0, 9ull, 0.000000000000000001},
    {0ll, 0.0, 0ull, 0.0000000000000000001},
    {0ll, 0.0, 0ull, 0.00000000000000000001},
};

// The per-vector constants, read in front of the barrier: ALP_RD = the rowgroup's dictionary (RdDict, alp_device.hpp); ALP vectors use
// the same two words for lo = FACT_ARR[f], hi = bits of FRAC_ARR[e] — table reads that depend only on the descriptor.
// (plus, for ALP, 10^f as a double and the no-wrap limit of the conversion shortcut: every table read that depends on the descriptor is in
// flight with the packed words instead of behind the barrier)
struct VectorConsts {
	uint64_t lo, hi;
	uint64_t fact_d_bits, shortcut_bound;
};
__device__ __forceinline__ VectorConsts load_vector_consts(const alpgpu_rowgroup_state* __restrict__ rgs, uint64_t v, const alpgpu_vector_desc& d) {
	if (d.scheme != ALPGPU_SCHEME_ALP) { // wave-uniform
		const RdDict r = load_rd_dict(rgs, v, true);
		return VectorConsts {r.lo, r.hi, 0ull, 0ull};
	}
	const DecodeTabEntry& by_f = kDecodeTab[d.f];
	return VectorConsts {static_cast<uint64_t>(by_f.fact), static_cast<uint64_t>(__double_as_longlong(kDecodeTab[d.e].frac)),
	                     static_cast<uint64_t>(__double_as_longlong(by_f.fact_d)), by_f.shortcut_bound};
}

// Where the packed words of a vector are read from: the workgroup's LDS stage (the column kernels), or HBM directly (k_sink_direct).
struct WordPair {
	ulonglong2 w0, w1;
};
struct StagedWords {
	const uint8_t* stage;
	__device__ __forceinline__ WordPair pair(int i) const { // units i and i + 8: stream words k and k + 1 of a column pair
		return WordPair {reinterpret_cast<const ulonglong2*>(stage)[i], reinterpret_cast<const ulonglong2*>(stage)[i + 8]};
	}
	__device__ __forceinline__ uint2 left_pair(int rbw, int i) const { // left words i and i + 32
		return make_uint2(reinterpret_cast<const uint32_t*>(stage + 128 * rbw)[i], reinterpret_cast<const uint32_t*>(stage + 128 * rbw)[i + 32]);
	}
};
struct BufferWords { // HBM through buffer loads (staged_decode.hpp: packed_word_resources); the second unit of a pair is the first one's address with an immediate offset
	__amdgpu_buffer_rsrc_t units, lefts;
	__device__ __forceinline__ WordPair pair(int i) const {
		typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
		const uint32_t at = static_cast<uint32_t>(i) * 16u;
		const u32x4    a = __builtin_amdgcn_raw_buffer_load_b128(units, at, 0, 0);
		const u32x4    b = __builtin_amdgcn_raw_buffer_load_b128(units, at, 128, 0); // unit i + 8: the same address register, a scalar offset
		return WordPair {make_ulonglong2((static_cast<uint64_t>(a[1]) << 32) | a[0], (static_cast<uint64_t>(a[3]) << 32) | a[2]),
		                 make_ulonglong2((static_cast<uint64_t>(b[1]) << 32) | b[0], (static_cast<uint64_t>(b[3]) << 32) | b[2])};
	}
	__device__ __forceinline__ uint2 left_pair(int, int i) const {
		const uint32_t at = static_cast<uint32_t>(i) * 4u;
		return make_uint2(__builtin_amdgcn_raw_buffer_load_b32(lefts, at, 0, 0), __builtin_amdgcn_raw_buffer_load_b32(lefts, at, 128, 0));
	}
};

template <int V>
struct ExcMode {
	static constexpr int value = V;
};
template <int A> // 0: the literal arithmetic, 1: the IEEE-product shortcut on 64-bit fields, 2: the same on fields of <= 32 bits (32-bit unpack)
struct ArithShortcut {
	static constexpr int value = A;
};
// N_Q consecutive quarters of one vector, from quarter q0 on (a quarter = steps kStepsPerWave q .. + kStepsPerWave - 1 = what one wavefront of a
// four-wavefront workgroup does; the sinks accumulate quarter q0 + i into acc[i]).  `em` = the vector's exception mask as this wavefront sees
// it (ignored when the vector has none), L = where staged exception values live.
// ONLY: 0 = either scheme (decided from the descriptor), 1 = the caller knows the vector is ALP, 2 = ALP_RD (only that arm is compiled in).
template <bool NT_STORE, int SINK, int N_Q, int ONLY = 0, class LDS, class WORDS>
__device__ __forceinline__ void decode_vector_quarters(const LDS& L, const WORDS& units, const alpgpu_vector_desc& d, const VectorConsts& dict, const ExcMask& em,
                                                      const uint8_t* __restrict__ rec, double2* __restrict__ dst, int q0, int lane, double* acc,
                                                       double range_lo, double range_hi) {
	const int      bw       = d.bw;
	const int      cnt      = d.exc_cnt;
	const bool     all_staged = cnt <= static_cast<int>(LDS::kExcBytes) / (d.scheme == ALPGPU_SCHEME_ALP ? 8 : 2); // wave-uniform
	const int      a        = lane & 7;
	const int      r0       = lane >> 3;
	// The pair (row, columns 2a, 2a + 1) out of its two stream words (alp_device.hpp: unpack_pair_u64), in two halves: the reads of a whole
	// batch of steps are requested before the first of them is used — with the words in HBM (k_sink_direct) every step is otherwise its own
	// dependent round trip.
	constexpr int kSteps = N_Q * kStepsPerWave;
	constexpr int kBatch = kSteps < kDecodeBatch ? kSteps : kDecodeBatch;
	constexpr int kBatchRd = ONLY == 2 ? 1 : (kSteps < 2 ? kSteps : 2); // ALP_RD keeps the left words and the dictionary selects in registers as well
	auto request = [&](int width, int row) { return units.pair(8 * ((row * width) >> 6) + a); };
	auto extract = [&](int width, uint64_t wmask, int row, const WordPair w) {
		const int s = (row * width) & 63;
		U64Pair   r;
		r.x = ((w.w0.x >> s) | ((w.w1.x << 1) << (63 - s))) & wmask; // (w1 << (64 - s)) without the undefined shift by 64 when s == 0
		r.y = ((w.w0.y >> s) | ((w.w1.y << 1) << (63 - s))) & wmask;
		return r;
	};
	if (ONLY == 1 || (ONLY == 0 && d.scheme == ALPGPU_SCHEME_ALP)) {
		const uint64_t base = static_cast<uint64_t>(d.base);
		const int64_t  fact = static_cast<int64_t>(dict.lo);
		const double   frac = __longlong_as_double(static_cast<long long>(dict.hi));
		const uint64_t mask = bw_mask(bw);
		// Conversion shortcut, decided once per vector from its descriptor.  If every value base + digit of this vector
		// lies in (-2^51, 2^51) and times 10^f stays inside int64, then
		//   * (double)value is exact and equals  bitcast(bits(2^52+2^51) + value) - (2^52+2^51)   (one 64-bit add, one f64 add),
		//   * (double)(int64)(value * 10^f) is the correctly rounded product of two exactly representable doubles,
		//     i.e. the IEEE product  (double)value * 10^f,
		// which replaces the 64-bit integer multiply and the software int64->double conversion (src/falp.cpp:114-121 does
		// them per value) and yields the same bits.  Anything else takes the literal path.
		// (decided in integers on wave-uniform values against ONE table entry, kDecodeTab: as doubles — two software int64 -> double
		//  conversions, |.|, max, a product — the decision alone was ~35 vector instructions per wavefront and vector)
		const int64_t  lo       = d.base;
		const int64_t  bound    = static_cast<int64_t>(dict.shortcut_bound); // <= 2^51 - 1
		const double   fact_d   = __longlong_as_double(static_cast<long long>(dict.fact_d_bits));
		// |lo| <= bound first: lo + mask cannot overflow then (mask < 2^50); lo <= lo + mask, so the two ends bound everything between
		const bool     shortcut = bw <= 50 && lo >= -bound && lo <= bound && static_cast<int64_t>(static_cast<uint64_t>(lo) + mask) <= bound;
		const uint64_t kbits   = 0x4338000000000000ull + base;
		// what follows the conversion of a pair: exceptions patched in, then the sink.
		// EXC (compile time): 0 = the vector has no exceptions: nothing is looked up; 1 = it has some and all of their values are staged in LDS: no
		// memory load anywhere in the loop; 2 = decided per step at run time (cnt > 0, staged or not) — the form every caller had until round 5.
		// Why the first two exist (round 5): with the rare "value beyond the stage -> load it from HBM" arm inside the loop the compiler places
		// s_waitcnt vmcnt(0) at the join in front of EVERY step's store — on gfx9 stores count in vmcnt, so each store of a wavefront waited for
		// the acknowledgement of the one before it, exceptions or not — and every step was a basic block of its own.  The store decode now picks
		// the loop per vector (wave-uniform); the sinks (register budgets tuned around the old form) stay on 2.
		auto finish_pair = [&](auto exc_mode, int m, double ox, double oy, double* acc_q) {
			constexpr int EXC = decltype(exc_mode)::value;
			if (EXC == 1 || (EXC == 2 && cnt > 0)) {
				const bool     staged = EXC == 1 ? true : all_staged;
				int            rank;
				uint32_t       hits;
				if constexpr (LDS::kPrefixInLds) { hits = exception_hits_lds(L, m, lane, rank); } else { hits = exception_hits(em, m, lane, rank); }
				if (hits & 1u) {
					ox = __longlong_as_double(static_cast<long long>(fetch_exception<8>(L, rec, rank, staged)));
					++rank;
				}
				if (hits & 2u) { oy = __longlong_as_double(static_cast<long long>(fetch_exception<8>(L, rec, rank, staged))); }
			}
			if constexpr (SINK != kSinkStore) {
				consume_pair<SINK>(ox, oy, acc_q, range_lo, range_hi);
			} else {
				store_pair<NT_STORE>(dst + 64 * m + lane, ox, oy);
			}
		};
		// ArithShortcut<2> (round 5; the store decode's vectors of <= 32 bits on the shortcut route — narrow vectors are bound by their vector
		// instructions, not by HBM: profiles/r05_decode_exceptions.txt): the field lies in three of the four dwords of its two stream words and
		// comes out with ONE 32-bit funnel shift (v_alignbit_b32; the amount is taken modulo 32) where the 64-bit form takes three 64-bit shifts;
		// and (double)(base + digit) is the double whose bits are {0x43380000, digit} = M + digit (M = 2^52 + 2^51) minus the wave-uniform double
		// M - base, whose bits are bits(M) - base (scalar integer arithmetic; |base| < 2^51 is the shortcut's condition) — every quantity an
		// integer below 2^53, the difference exact — one v_add_f64 where the 64-bit form adds the base in integers (two instructions) first.
		// The same value, hence the same bits, as ArithShortcut<1>: 7 vector instructions per value instead of 13.
		const uint32_t mask32   = static_cast<uint32_t>(mask);
		const double   magic_mb = __longlong_as_double(static_cast<long long>(0x4338000000000000ull - static_cast<uint64_t>(lo))); // M - base
		auto alp_steps = [&](auto exc_mode, auto shortcut_arith) {
			constexpr int SHORT = static_cast<int>(decltype(shortcut_arith)::value);
#pragma unroll
			for (int b = 0; b < kSteps; b += kBatch) {
				WordPair w[kBatch];
#pragma unroll
				for (int i = 0; i < kBatch; ++i) { w[i] = request(bw, 8 * (kStepsPerWave * q0 + b + i) + r0); }
#pragma unroll
				for (int i = 0; i < kBatch; ++i) {
					const int     m = kStepsPerWave * q0 + b + i;
					if constexpr (SHORT == 2) {
						const uint32_t sft = static_cast<uint32_t>((8 * m + r0) * bw) & 63u;
						const bool     low = sft < 32u; // the field begins in the first dword of word k (else in the second; it ends at most one dword later)
						const uint32_t x0 = static_cast<uint32_t>(w[i].w0.x), x1 = static_cast<uint32_t>(w[i].w0.x >> 32), x2 = static_cast<uint32_t>(w[i].w1.x);
						const uint32_t y0 = static_cast<uint32_t>(w[i].w0.y), y1 = static_cast<uint32_t>(w[i].w0.y >> 32), y2 = static_cast<uint32_t>(w[i].w1.y);
						const uint32_t ux = __builtin_amdgcn_alignbit(low ? x1 : x2, low ? x0 : x1, sft) & mask32;
						const uint32_t uy = __builtin_amdgcn_alignbit(low ? y1 : y2, low ? y0 : y1, sft) & mask32;
						const double   dx = __longlong_as_double(static_cast<long long>(0x4338000000000000ull | ux)) - magic_mb;
						const double   dy = __longlong_as_double(static_cast<long long>(0x4338000000000000ull | uy)) - magic_mb;
						finish_pair(exc_mode, m, (dx * fact_d) * frac, (dy * fact_d) * frac, sink_acc<SINK>(acc, (b + i) / kStepsPerWave));
						continue;
					}
					const U64Pair u = extract(bw, mask, 8 * m + r0, w[i]);
					if constexpr (SHORT == 1) {
						finish_pair(exc_mode, m, ((__longlong_as_double(static_cast<long long>(u.x + kbits)) - kMagic) * fact_d) * frac,
						            ((__longlong_as_double(static_cast<long long>(u.y + kbits)) - kMagic) * fact_d) * frac, sink_acc<SINK>(acc, (b + i) / kStepsPerWave));
					} else {
						finish_pair(exc_mode, m, decode_value(static_cast<int64_t>(u.x + base), fact, frac), decode_value(static_cast<int64_t>(u.y + base), fact, frac),
						            sink_acc<SINK>(acc, (b + i) / kStepsPerWave));
					}
				}
			}
		};
		constexpr bool kPerVectorLoops = SINK == kSinkStore && N_Q == 1;
		const bool narrow32 = kPerVectorLoops && bw <= 32;
		if (shortcut) { // wave-uniform; ONE branch per vector, not one per step (scalar instructions are the scarce ones here)
			if (kPerVectorLoops && cnt == 0) {
				if (narrow32) {
					alp_steps(ExcMode<0> {}, ArithShortcut<2> {});
				} else {
					alp_steps(ExcMode<0> {}, ArithShortcut<1> {});
				}
			} else if (kPerVectorLoops && all_staged) {
				if (narrow32) {
					alp_steps(ExcMode<1> {}, ArithShortcut<2> {});
				} else {
					alp_steps(ExcMode<1> {}, ArithShortcut<1> {});
				}
			} else {
				// round 6, call 36: the SINKS' vectors of <= 32 bits through the 32-bit unpack too (7 vector instructions per value instead of 13; until
				// then the store decode's only): SUM of 2-24-bit columns 0.54-0.76 -> 0.45-0.69 ms per 1 Mi vectors (-9 to -15 %), with 20 exceptions per vector -8 to -13 %,
				// the benchmark column -3 %; same bits.
				if (!kPerVectorLoops && bw <= 32) {
					alp_steps(ExcMode<2> {}, ArithShortcut<2> {});
				} else {
					alp_steps(ExcMode<2> {}, ArithShortcut<1> {});
				}
			}
		} else {
			alp_steps(ExcMode<2> {}, ArithShortcut<0> {});
		}
	} else {
		// ALP_RD: right parts = u64 lanes (bw = rbw, base 0); left parts = u16 lanes, 64 streams x 16 rows (value i ->
		// lane64 = i & 63, row = i >> 6, word k at left[64*k + lane64]); a lane's pair shares the row 2m + (lane >> 5)
		// and is one aligned u32 of the left stream.
		const int      rbw  = bw;
		const int      lbw  = d.lbw;
		const uint64_t mask = bw_mask(rbw);
		const uint32_t lmsk = (1u << lbw) - 1u;
		const uint64_t dlo = dict.lo, dhi = dict.hi;
		(void)dlo, (void)dhi;
		auto rd_steps = [&](auto exc_mode) {
			constexpr int EXC = decltype(exc_mode)::value; // as in the ALP arm
#pragma unroll
			for (int b = 0; b < kSteps; b += kBatchRd) {
				WordPair rw[kBatchRd];
				uint2    lw[kBatchRd];
#pragma unroll
				for (int i = 0; i < kBatchRd; ++i) {
					const int m = kStepsPerWave * q0 + b + i;
					rw[i]       = request(rbw, 8 * m + r0);
					lw[i]       = units.left_pair(rbw, 32 * (((2 * m + (lane >> 5)) * lbw) >> 4) + (lane & 31));
				}
#pragma unroll
				for (int i = 0; i < kBatchRd; ++i) {
					const int      m   = kStepsPerWave * q0 + b + i;
					double*        acc_q = sink_acc<SINK>(acc, (b + i) / kStepsPerWave);
					U64Pair        u   = extract(rbw, mask, 8 * m + r0, rw[i]);
					if constexpr (ONLY == 2) { asm volatile("" : "+v"(u.x), "+v"(u.y)); } // (k_sink_direct) the right parts extracted HERE: their four words die before the left parts' work begins
					const int      s   = ((2 * m + (lane >> 5)) * lbw) & 15;
					const uint32_t w0 = lw[i].x, w1 = lw[i].y;
					const uint32_t i0  = (((w0 & 0xFFFFu) >> s) | ((w1 & 0xFFFFu) << (16 - s))) & lmsk;
					const uint32_t i1  = (((w0 >> 16) >> s) | ((w1 >> 16) << (16 - s))) & lmsk;
					uint64_t       l0  = L.rdict[i0 & 7u];
					uint64_t       l1  = L.rdict[i1 & 7u];
					if (EXC == 1 || (EXC == 2 && cnt > 0)) {
						const bool     staged = EXC == 1 ? true : all_staged;
						int            rank;
						uint32_t       hits;
						if constexpr (LDS::kPrefixInLds) { hits = exception_hits_lds(L, m, lane, rank); } else { hits = exception_hits(em, m, lane, rank); }
						if (hits & 1u) {
							l0 = fetch_exception<2, uint64_t>(L, rec, rank, staged);
							++rank;
						}
						if (hits & 2u) { l1 = fetch_exception<2, uint64_t>(L, rec, rank, staged); }
					}
					const double ox = __longlong_as_double(static_cast<long long>((l0 << rbw) | u.x));
					const double oy = __longlong_as_double(static_cast<long long>((l1 << rbw) | u.y));
					if constexpr (SINK != kSinkStore) {
						consume_pair<SINK>(ox, oy, acc_q, range_lo, range_hi);
						if constexpr (ONLY == 2 && SINK == kSinkMinMax) { asm volatile("" : "+v"(acc_q[1])); }
						if constexpr (ONLY == 2) { asm volatile("" : "+v"(*acc_q)); } // ... and the pair added HERE: left to itself the compiler keeps all sixteen results for the end (208 bytes of scratch, 3.7 x the time)
					} else {
						store_pair<NT_STORE>(dst + 64 * m + lane, ox, oy);
					}
				}
				if constexpr (ONLY == 2) { asm volatile("" ::: "memory"); } // (k_sink_direct) the next step's requests stay behind this one's use
			} // batch
		};
		constexpr bool kPerVectorLoops = SINK == kSinkStore && N_Q == 1;
		if (kPerVectorLoops && cnt == 0) {
			rd_steps(ExcMode<0> {});
		} else if (kPerVectorLoops && all_staged) {
			rd_steps(ExcMode<1> {});
		} else {
			rd_steps(ExcMode<2> {});
		}
	}
}

// one wavefront's share of a staged vector (the column kernels: four wavefronts per vector)
template <bool NT_STORE, int SINK = kSinkStore, class LDS = DecodeLds>
__device__ __forceinline__ void decode_staged_vector(const LDS& L, const alpgpu_vector_desc& d, const VectorConsts& dict,
                                                     const uint8_t* __restrict__ rec, double2* __restrict__ dst, int wave, int lane, double* acc = nullptr,
                                                     double range_lo = 0.0, double range_hi = 0.0) {
	ExcMask em {0u, 0};
	if (d.exc_cnt > 0) { em = load_exception_mask(L, lane); }
	decode_vector_quarters<NT_STORE, SINK, 1>(L, StagedWords {L.stage}, d, dict, em, rec, dst, wave, lane, acc, range_lo, range_hi);
}

// V consecutive vectors per workgroup: all of their loads are in flight together, then they are unpacked one after the
// other by the same 4 wavefronts.  V = 2 doubles the bytes in flight per CU for the same residency (8 workgroups per CU).
template <int V, bool NT_STORE, int SINK = kSinkStore, class LDS = DecodeLds>
__global__ __launch_bounds__(64 * kDecWaves) void k_decode_column(const alpgpu_vector_desc* __restrict__ descs,
                                                                  const alpgpu_rowgroup_state* __restrict__ rgs,
                                                                  const uint8_t* __restrict__ packed,
                                                                  const uint8_t* __restrict__ excs, double* __restrict__ out,
                                                                  uint64_t n_vectors, uint64_t wg_offset, double lo, double hi, uint32_t gate_word,
                                                                  uint64_t* __restrict__ progress, uint64_t progress_tag) {
	static_assert(LDS::kStage == kStageBytes || SINK == kSinkStore, "the sinks pass their lane partials through a full stage");
	__shared__ LDS L[V];
	const int      tid  = static_cast<int>(threadIdx.x);
	const int      lane = tid & 63;
	const int      wave = wave_in_wg();
	const uint64_t v0   = (wg_offset + blockIdx.x) * V;
	if (v0 >= n_vectors) { return; }
	// An unhinted decode (api_decode.hip) launches every candidate shape; the plan kernel in front of them has written which one runs (bits 8.. of gate_word
	// = this launch's number, 0 = not a candidate: the usual launch).  One scalar load, taken by candidates only; a closed candidate costs its dispatch.
	if (SINK == kSinkStore && (gate_word >> 8) != 0u) { // (kernel argument: uniform)
		if (progress[kCtxWordShape] != static_cast<uint64_t>(gate_word >> 8)) { return; }
	}
	// the read-ahead's pace (read_ahead_kernels.hip): workgroups are dispatched in ascending order, every 128th says where the launch is
	if (SINK == kSinkStore && progress != nullptr && (blockIdx.x & 127u) == 0 && tid == 0) {
		__hip_atomic_store(progress, progress_tag | v0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}

	alpgpu_vector_desc d[V];
	VectorConsts       dict[V];
	stage_vectors<8>(L, d, dict, descs, packed, excs, v0, n_vectors, tid, wave, [&](uint64_t v, const alpgpu_vector_desc& dv) { return load_vector_consts(rgs, v, dv); });

	if constexpr (SINK != kSinkStore) {
		double acc[V];
#pragma unroll
		for (int i = 0; i < V; ++i) {
			acc[i] = 0.0;
			if (v0 + i < n_vectors) {
				if constexpr (SINK == kSinkProbe) {
					const int       n_units = 8 * (d[i].bw + (d[i].scheme == ALPGPU_SCHEME_ALP ? 0 : d[i].lbw));
					const uint64_t* st      = reinterpret_cast<const uint64_t*>(L[i].stage);
					uint64_t        sum     = 0;
					for (int c = tid; c < n_units; c += 64 * kDecWaves) { sum += st[2 * c] + st[2 * c + 1]; }
					acc[i] = static_cast<double>(sum & 0xFFFFFu);
				} else {
					decode_staged_vector<NT_STORE, SINK>(L[i], d[i], dict[i], excs + d[i].exc_off, nullptr, wave, lane, &acc[i], lo, hi);
				}
			}
		}
		finish_vector_sinks<SINK == kSinkCount>(L, acc, out, v0, n_vectors, wave, lane, [](int, double&) {});
		return;
	}
#pragma unroll
	for (int i = 0; i < V; ++i) {
		if (v0 + i < n_vectors) {
			decode_staged_vector<NT_STORE, kSinkStore, LDS>(L[i], d[i], dict[i], excs + d[i].exc_off, reinterpret_cast<double2*>(out + (v0 + i) * kVec), wave, lane);
		}
	}
}

// ---- the sinks with ONE wavefront per vector, packed words read from HBM as they are needed (no stage, no barrier) ---------------------
// What the four-wavefront sinks run out of is instruction issue — the scalar unit first, the VALU right behind — because every wavefront of a
// workgroup repeats the wave-uniform prologue of both its vectors (profiles/r03_consumers.txt).  Here a wavefront owns a vector: one
// prologue per vector, no cross-wavefront reduction, no barrier; without a stage its LDS is the exception mask and values only (1.2 KiB), so
// eight wavefronts per SIMD stay resident and hide the two dependent round trips (descriptor -> packed words) between them.  A lane reads
// the two 16-byte units of each of its eight pairs straight from HBM (buffer loads bounded to the vector's words): 16 loads per wavefront
// whatever the width; the 64 lanes of a load touch 8 runs of 128 bytes.  Results are bit-identical to k_decode_column's sinks: the lane keeps the four quarter partials p[q][L] apart,
// then (p0 + p1) + (p2 + p3), then the adjacent-lane tree (include/alpgpu.h).
constexpr int kSinkDirectOcc = 8; // wavefronts per SIMD the register budget is sized for (8 -> <= 64 VGPRs; measured against 5 and 6: profiles/r03_consumers.txt)
constexpr int kSinkStage = 3584; // bytes of packed words (bit widths <= 28) a wavefront of k_sink_direct stages in its LDS by LDS-DMA; with mask, values and prefixes 4992 B per wavefront = eight workgroups per CU (0: none)
constexpr int kSinkStageMaxExc = 48; // ... only for vectors with at most this many exceptions
struct __attribute__((aligned(16))) SinkWaveLds {
	static constexpr bool kPrefixInLds = true; // exception_hits_lds
	uint8_t  stage[kSinkStage + 128]; // + the unit row past the end that the unpack reads and masks off
	uint32_t mask[32];
	static constexpr uint32_t kExcBytes = kExcStageBytes;
	uint8_t  excv[kExcStageBytes];
	uint32_t pref[32]; // exceptions in front of mask word i
	uint16_t rdict[8]; // ALP_RD: the rowgroup's dictionary (DecodeLdsT)
};
template <int SINK>
__global__ __launch_bounds__(64 * kDecWaves, kSinkDirectOcc) void k_sink_direct(const alpgpu_vector_desc* __restrict__ descs, const alpgpu_rowgroup_state* __restrict__ rgs,
                                                                   const uint8_t* __restrict__ packed, const uint8_t* __restrict__ excs, double* __restrict__ out,
                                                                   uint64_t n_vectors, uint64_t wg_offset, double lo, double hi) {
	// gfx950 range-checks the single-register AMOUNT of a 64-bit shift (v_lshrrev_b64 / v_lshlrev_b64, which this kernel lives on) as a register
	// PAIR: in the LAST register of the allocation it counts as out of range and VGPR0 is read instead (tools/last_vgpr_probe.hip).  Builds
	// of this kernel whose 64 registers were all in use with a shift amount in v63 returned wrong sums for ~5 % of some vectors; the
	// register allocator does not know the rule.  tools/check_top_vgpr.py (run by tests/test_build_rules.py) looks for the pattern in every
	// kernel of every build; -DALPGPU_SINK_REGISTER_MARGIN allocates one register more than the kernel uses instead (72 registers, 7
	// wavefronts per SIMD, 3-6 % slower: measured in profiles/r03_consumers.txt), which makes the pattern impossible here.
#ifdef ALPGPU_SINK_REGISTER_MARGIN
	asm volatile("" ::: "v64");
#endif
	__shared__ SinkWaveLds S[kDecWaves];
	const int      lane = static_cast<int>(threadIdx.x) & 63;
	const int      wave = wave_in_wg();
	const uint64_t v    = (wg_offset + blockIdx.x) * kDecWaves + wave;
	if (v >= n_vectors) { return; } // wave-uniform; no barrier anywhere in this kernel
	SinkWaveLds&             L    = S[wave];
	const alpgpu_vector_desc d    = descs[v];
	const VectorConsts       dict = load_vector_consts(rgs, v, d);
	const uint8_t*           rec  = excs + d.exc_off;
	const bool               is_alp = d.scheme == ALPGPU_SCHEME_ALP;
	const int                cnt  = d.exc_cnt;
	// staged: a narrow ALP vector with few exceptions
	const bool    staged = is_alp && 128u * d.bw <= static_cast<uint32_t>(kSinkStage) && cnt <= kSinkStageMaxExc; // wave-uniform
	const ExcMask em     = stage_wave_vector<8>(L, d, packed, rec, staged, lane);
	const BufferWords words = packed_word_resources<BufferWords>(packed + d.packed_off, d.bw, d.lbw, is_alp);
	if (!is_alp) { // wave-uniform: the dictionary into the wavefront's LDS
		if (lane < 4) { stage_rd_dictionary(L, dict, lane); }
		wave_lds_sync();
	}
	double part[kDecWaves] = {0.0, 0.0, 0.0, 0.0};
	if constexpr (SINK == kSinkMinMax) { // part[0] / part[1]: the lane's minimum / maximum, from the empty interval
		part[0] = __builtin_inf();
		part[1] = -__builtin_inf();
	}
	if (staged) {
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		wave_lds_sync();
		decode_vector_quarters<false, SINK, kDecWaves, 1>(L, StagedWords {L.stage}, d, dict, em, rec, nullptr, 0, lane, part, lo, hi);
	} else
	if (is_alp) { // wave-uniform
		decode_vector_quarters<false, SINK, kDecWaves, 1>(L, words, d, dict, em, rec, nullptr, 0, lane, part, lo, hi);
	} else {
		// ALP_RD a quarter at a time: the right AND left words of eight steps in flight at once do not fit this kernel's 64 registers; with the two
		// pins in decode_vector_quarters' ALP_RD arm nothing is spilled (1.41 ms per 1 Mi vectors of an all-ALP_RD column, staged kernel 1.51;
		// without them 208 bytes of scratch and 5.4 ms)
#pragma unroll
		for (int q = 0; q < kDecWaves; ++q) {
			decode_vector_quarters<false, SINK, 1, 2>(L, words, d, dict, em, rec, nullptr, q, lane, sink_acc<SINK>(part, q), lo, hi);
			asm volatile("" ::: "memory"); // the next quarter's requests stay behind this one's use
		}
	}
	if constexpr (SINK == kSinkMinMax) { // the record {min, max}: one 16-byte store per vector
		wave_minmax_f64(part[0], part[1]);
		if (lane == 0) { reinterpret_cast<double2*>(out)[v] = make_double2(part[0], part[1]); }
		return;
	}
	static_assert(kDecWaves == 4, "the documented summation order is for 4 quarters per vector");
	store_vector_result<SINK == kSinkCount>(out, v, (part[0] + part[1]) + (part[2] + part[3]), lane);
}


int launch_sink_direct(hipStream_t stream, const alpgpu_column* col, double lo, double hi, void* d_out, bool count) {
	double* out = static_cast<double*>(d_out);
	if (count) { return launch_over_column(k_sink_direct<kSinkCount>, wgs_of(col, kDecWaves), dec_block(), 0, stream, col, out, lo, hi); }
	return launch_over_column(k_sink_direct<kSinkSum>, wgs_of(col, kDecWaves), dec_block(), 0, stream, col, out, 0.0, 0.0);
}

// d_zones[v] = {min, max} of vector v's decoded values, NaNs ignored (include/alpgpu.h: zone maps); n_vectors > 0
int launch_zone_map(hipStream_t stream, const alpgpu_column* col, void* d_zones) {
	return launch_over_column(k_sink_direct<kSinkMinMax>, wgs_of(col, kDecWaves), dec_block(), 0, stream, col, static_cast<double*>(d_zones), 0.0, 0.0);
}

int launch_decode_column(hipStream_t stream, const alpgpu_column* col, double* d_out, const DecodeShape& shape, int n_cus, uint64_t* progress, uint64_t progress_tag, uint32_t gate) {
	(void)n_cus;
	const uint32_t gate_word = gate != 0 && progress != nullptr ? gate << 8 : 0u; // (k_decode_column: a candidate launch of an unhinted decode)
	const bool     nt       = !shape.plain_stores;
	const int      V        = shape.vectors_per_wg == 1 ? 1 : 2;
	// Unused dynamic LDS that caps the workgroups resident per CU (shape.pad_kib).  Wide vectors want FEWER
	// streams in flight per CU than the eight the wavefront slots allow: a column of 40-53-bit vectors decodes at 0.81 of the HBM peak with six
	// workgroups per CU and at 0.75 with eight, 34-38 bits like seven; up to 33 bits eight are best (tools/sweep_residency.py,
	// profiles/r04_decode_floor.txt section 6).  policy_shape_f64 (decode_policy.hpp) sets it from the column's size hints.
	const unsigned pad_lds  = shape.pad_kib > 0 ? static_cast<unsigned>(shape.pad_kib) * 1024u : 0u;
	const auto launch = [&](auto kernel) { return launch_over_column(kernel, wgs_of(col, V), dec_block(), pad_lds, stream, col, d_out, 0.0, 0.0, gate_word, progress, progress_tag); };
	if (V == 2 && nt) { return launch(k_decode_column<2, true>); }
	if (V == 2) { return launch(k_decode_column<2, false>); }
	if (shape.many_exc && nt) { return launch(k_decode_column<1, true, kSinkStore, DecodeLdsManyExc>); } // one vector per workgroup, the 256-entry exception stage (columns of exception-heavy vectors)
	if (nt) { return launch(k_decode_column<1, true>); }
	return launch(k_decode_column<1, false>);
}

// vectors_per_wg in {1, 2}.  There is no output stream to compete with, so two vectors in flight per workgroup is the default
// (measured on the benchmark column: 1.39 / 1.16 / 1.43 ms for 1 / 2 / 4 vectors per workgroup).
int launch_decode_sum(hipStream_t stream, const alpgpu_column* col, double* d_sums, int vectors_per_wg) {
	if (vectors_per_wg == 1) { return launch_over_column(k_decode_column<1, false, kSinkSum>, wgs_of(col, 1), dec_block(), 0, stream, col, d_sums, 0.0, 0.0, 0u, kNoProgress, 0ull); }
	return launch_over_column(k_decode_column<2, false, kSinkSum>, wgs_of(col, 2), dec_block(), 0, stream, col, d_sums, 0.0, 0.0, 0u, kNoProgress, 0ull);
}

// measurement aid: the fused consumers' loads, barrier and reduction with the unpack left out (two vectors per workgroup, like them)
int launch_decode_probe(hipStream_t stream, const alpgpu_column* col, double* d_sums) {
	return launch_over_column(k_decode_column<2, false, kSinkProbe>, wgs_of(col, 2), dec_block(), 0, stream, col, d_sums, 0.0, 0.0, 0u, kNoProgress, 0ull);
}

// per-vector number of values in [lo, hi]: the same kernel with the predicate as its consumer (two vectors per workgroup)
int launch_decode_count_range(hipStream_t stream, const alpgpu_column* col, double lo, double hi, uint32_t* d_counts) {
	return launch_over_column(k_decode_column<2, false, kSinkCount>, wgs_of(col, 2), dec_block(), 0, stream, col, reinterpret_cast<double*>(d_counts), lo, hi, 0u, kNoProgress, 0ull);
}

} // namespace alpgpu
