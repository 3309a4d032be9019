// decode_policy.hpp — the store decode's LAUNCH RULE, whole: which kernel decodes a column (or a run of one), in what shape, and whether the read-ahead runs beside it.
// Pure functions of numbers — sizes (ColumnSizes) and options (DecodeOptions) in, a typed DecodeShape and "reads ahead" out — that the host (api_decode.hip, which keeps
// the state), the device (guard_kernels.hip: k_unhinted_plan) and a plain C++ program (tests/cpp/decode_policy_test.cpp: the rule is tested without a GPU) all evaluate.
// policy_decode_plan serves columns whose sizes the host knows (packed_bytes_hint / exc_bytes_hint, alpgpu_column_totals); policy_unhinted is its deliberate coarsening
// to three candidates for a column decoded right behind its encode, without the host synchronisation alpgpu_column_totals is: the sizes are then summed on the stream and
// the rule is evaluated THERE; what it decides reaches the decode launches as a word of context memory (round 6).  Both are made of the same named
// predicates.  Every threshold is a measured crossover: DESIGN.md §3.1, profiles/r05_read_ahead.txt, profiles/r06_decode_policy.txt.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace alpgpu {

// ---- words of the context's device memory (alpgpu_ctx::d_progress, 2 KiB = 256 words) ----
constexpr int kCtxWordProgress  = 0;  // the running decode's position, tagged (read_ahead_kernels.hip)
constexpr int kCtxWordHole      = 1;  // never written (what keeps the read-ahead's loads)
constexpr int kCtxWordBatches   = 2;  // batches of 64 vectors the read-ahead has read since the context was created (debug counter: alpgpu_debug_read_ahead_batches)
constexpr int kCtxWordShape     = 3;  // unhinted decode: the candidate launch that runs (1-based; the others leave at once)
constexpr int kCtxWordLead      = 4;  // unhinted decode: the read-ahead's lead_min (low word) and lead_max (high word), in vectors; 0 = no read-ahead
constexpr int kCtxWordPace      = 5;  // unhinted decode: picoseconds per vector (low word), widest record read ahead in packed bits (high word)
constexpr int kCtxWordTotals    = 8;  // unhinted decode: packed bytes, exceptions, ALP_RD vectors of the whole column (three words)
constexpr int kCtxWordSegments  = 64; // per-segment sums: 3 words each, up to 32 segments (guard_kernels.hip: k_segment_sums)

// ---- double columns ----
constexpr double   kReadAheadBits    = 6.5;    // the read-ahead pays up to this many packed bits per value on average without exceptions ...
constexpr double   kReadAheadBitsExc = 7.5;    // ... and with exceptions
constexpr uint64_t kReadAheadVectors = 262144; // shorter columns: the cold start and the join of the second stream eat the gain
constexpr double   kTwoVectorsBits    = 17.5;  // two vectors per workgroup up to here without exceptions ...
constexpr double   kTwoVectorsBitsExc = 22.0;  // ... and with (about two or more per vector)
constexpr double   kEmptyVectorsBits    = 0.75; // columns of (almost) nothing but 0-bit vectors: one vector per workgroup, six workgroups per CU, no read-ahead (call 2, the gov26 column)
// ---- float columns (a vector is 4 KiB; two per workgroup are the bytes in flight of one double vector): tools/sweep_f32_decode.py, profiles/r06_float_decode.txt ----
// Measured (call 1b, 1 Mi float vectors, fractions of 8 TB/s): cold, two vectors per workgroup are ahead of one at every width and of four wherever there are exceptions; without
// exceptions four are 1-2 points ahead at 6-14 bits only (and at 1 bit): not worth a rule — always two.  The read-ahead lifts 2-7-bit columns from 0.49-0.60 to
// 0.60-0.63 (with exceptions 0.44-0.54 -> 0.51-0.54) and loses from 8 bits on and at 1 bit; leads of ~20 us beat the double rule's 30-50.
// Round 6, late: float columns of 2-8-bit vectors WITHOUT exceptions are streamed by persistent workgroups (decode_stream_f32_kernels.hip; shape 27: chunks of 12 vectors,
// 12 decoding + 2 loading wavefronts, one workgroup per CU) — 0.65-0.73 of the HBM peak against 0.60-0.65 for two vectors per workgroup + the read-ahead (calls 19-22).
// With ~2 or more exceptions per vector it is level or behind cold (0.51-0.53 against 0.53-0.55; ahead warm), from 9 bits on it sits on a plateau of 0.69-0.70 that
// the small workgroups pass, and a column of 1-bit vectors is faster as it was (0.76): the rule below.  ALPGPU_F32_STREAM_BITS=0: never.
constexpr double   kStreamBitsF32      = 8.5;
constexpr double   kStreamLeastBitsF32 = 1.5;
constexpr uint64_t kStreamVectorsF32   = 32768; // shorter columns: a few chunks per workgroup only
constexpr int      kStreamShapeF32     = 27;
__host__ __device__ inline bool policy_stream_f32(uint64_t n_vectors, double packed_bytes, bool with_exc) {
	const double n = static_cast<double>(n_vectors);
	return kStreamBitsF32 > 0.0 && n_vectors >= kStreamVectorsF32 && !with_exc && packed_bytes > kStreamLeastBitsF32 * 128.0 * n && packed_bytes <= kStreamBitsF32 * 128.0 * n;
}
constexpr double kReadAheadBitsF32     = 7.5;
constexpr double kReadAheadBitsExcF32  = 7.5;
constexpr double kFourVectorsBitsF32    = 0.0;     // four float vectors per workgroup up to here (two beyond)
constexpr double kFourVectorsBitsExcF32 = 0.0;

// ---- the predicates both rules are made of ----
constexpr double   kExcBytesPerVector     = 16.0;         // "with exceptions": about two or more per vector (16 bytes of record)
constexpr double   kManyExcBytesPerVector = 10.0 * 128.0; // exception-heavy: more exceptions per vector than the 128-entry stage holds, on average
constexpr double   kWideBits              = 38.0;         // wide vectors: a CU wants fewer than eight workgroups of them (the residency pads below)
constexpr uint64_t kReadAheadForcedVectors = 32768;       // the read-ahead asked for (ALPGPU_OPT_DECODE_READ_AHEAD = 1): any column long enough to be worth a second launch
// "the column's vectors carry exceptions" as far as the launch shape is concerned
__host__ __device__ inline bool policy_with_exceptions(double n_vectors, double exc_bytes) { return exc_bytes >= kExcBytesPerVector * n_vectors; }
// packed bits per value, on average
__host__ __device__ inline double policy_bits(uint64_t n_vectors, double packed_bytes) { return packed_bytes / (128.0 * (n_vectors > 0 ? static_cast<double>(n_vectors) : 1.0)); }
// More vectors per workgroup = more bytes in flight per CU, which is what narrow vectors lack (two dependent round trips for 8 KiB of
// output) and what wide ones pay for.  Crossovers measured at 1-bit resolution on 1 Mi-vector columns (tools/sweep_vpw_fine.py,
// profiles/r04_decode_floor.txt): without exceptions one vector per workgroup wins from 17 bits on (16 itself — whole KiB per vector —
// still prefers more), with ~2 or more exceptions per vector from 21 bits on; every ALP_RD column is far beyond either.
// (17.5: with the residency caps below two vectors per workgroup win through 17 bits; with exceptions through 22: round 5)
__host__ __device__ inline bool policy_narrow(double bits, bool with_exc) { return bits <= (with_exc ? kTwoVectorsBitsExc : kTwoVectorsBits); }
__host__ __device__ inline bool policy_empty(double bits) { return bits <= kEmptyVectorsBits; }
__host__ __device__ inline bool policy_wide(double bits) { return bits >= kWideBits; }
// more than half of the vectors belong to ALP_RD rowgroups (more arithmetic per value; far wider than any threshold here)
__host__ __device__ inline bool policy_mostly_rd(double n_vectors, double rd_vectors) { return 2.0 * rd_vectors > n_vectors; }
// ... from alpgpu_column::alp_rd_rowgroups_hint (ALP_RD rowgroups + 1; 0: unknown)
__host__ __device__ inline double policy_rd_vectors_of_hint(uint64_t rd_rowgroups_hint) { return rd_rowgroups_hint != 0 ? static_cast<double>(rd_rowgroups_hint - 1) * 100.0 : 0.0; }
// the widest vectors the read-ahead pays for when left to the library
__host__ __device__ inline double policy_read_ahead_bits(bool with_exc, int value_bytes) { return value_bytes == 8 ? (with_exc ? kReadAheadBitsExc : kReadAheadBits) : (with_exc ? kReadAheadBitsExcF32 : kReadAheadBitsF32); }

// ---- what a launch of the store decode looks like (launch.hpp: launch_decode_column, launch_decode_column_f32, launch_decode_stream_f32) ----
constexpr int kPadNone = -1;
enum DecodeFamily : int {
	kDecodeStaged     = 0, // k_decode_column / k_decode_column_f32: four wavefronts unpack vectors_per_wg vectors from an LDS stage
	kDecodeWaveDirect = 1, // float columns, ALPGPU_OPT_DECODE_VECTORS_PER_WG = 8: one wavefront per vector, no stage, no barrier (k_sink_direct_f32 as a store decoder)
	kDecodeStreamed   = 2, // float columns: persistent workgroups (decode_stream_f32_kernels.hip), stream_shape 16..30
};
struct DecodeShape {
	int  vectors_per_wg; // staged: 1 or 2 (float columns: 4 too); one wavefront per vector: the workgroup's 4; streamed: not used
	bool plain_stores;   // plain instead of non-temporal stores (ALPGPU_OPT_DECODE_PLAIN_STORES)
	bool many_exc;       // the instance with the 256-entry exception stage (decode_kernels.hip: DecodeLdsManyExc; double columns, one vector per workgroup, non-temporal stores)
	int  pad_kib;        // unused dynamic LDS per workgroup that caps the workgroups resident per CU; kPadNone: none
	int  family;         // DecodeFamily
	int  stream_shape;   // kDecodeStreamed: which (decode_stream_f32_kernels.hip: launch_decode_stream_f32); else 0
};
// the number alpgpu_decode_vectors_per_wg reports and ALPGPU_OPT_DECODE_VECTORS_PER_WG takes: 1, 2, 4; 8 = one wavefront per vector; 16..30 = streamed
__host__ __device__ inline int decode_shape_number(const DecodeShape& s) { return s.family == kDecodeStreamed ? s.stream_shape : (s.family == kDecodeWaveDirect ? 8 : s.vectors_per_wg); }
// THE word of alpgpu_debug_decode_plan (include/alpgpu.h), nowhere else.  double: bit 0 one vector per workgroup, bit 1 plain stores, bit 6 the 256-entry exception
// stage, bits 8.. the residency pad in KiB (none: 0); float: bits 0-7 decode_shape_number, bits 8.. the pad (none: 0xFF)
__host__ __device__ inline uint64_t decode_debug_word(const DecodeShape& s, int value_bytes) {
	if (value_bytes == 4) { return static_cast<uint64_t>(decode_shape_number(s) | ((s.pad_kib >= 0 ? s.pad_kib : 0xFF) << 8)); }
	return static_cast<uint64_t>((s.vectors_per_wg == 1 ? 1 : 0) | (s.plain_stores ? 2 : 0) | (s.many_exc ? 64 : 0) | ((s.pad_kib >= 0 ? s.pad_kib : 0) << 8));
}

// ---- what the rule is evaluated from ----
struct ColumnSizes { // of a column or a run of one; all 0: nothing known
	uint64_t n_vectors, packed_bytes, exc_bytes;
	double   rd_vectors; // vectors of ALP_RD rowgroups (policy_rd_vectors_of_hint)
};
struct DecodeOptions { // alpgpu_set_option (api_context.hip)
	int  forced_vpw;        // ALPGPU_OPT_DECODE_VECTORS_PER_WG: 0 = by the rule, else 1, 2, 4, 8, 16-30 (double columns run 4 as 2 and everything from 8 on as 1)
	int  forced_pad_kib;    // ALPGPU_OPT_DECODE_RESIDENCY_PAD: -1 = by the rule, else KiB (0 = never cap)
	int  read_ahead;        // ALPGPU_OPT_DECODE_READ_AHEAD: -1 = by the rule, 0 = never, 1 = wherever it can run
	bool streams_serialize; // kernels of two streams cannot run side by side in this process (api_context.hip): left to itself the library starts no read-ahead
	bool plain_stores;      // ALPGPU_OPT_DECODE_PLAIN_STORES
};

// the read-ahead on its own (ALPGPU_OPT_DECODE_READ_AHEAD = -1): long columns of narrow vectors only
__host__ __device__ inline bool policy_read_ahead_auto(uint64_t n_vectors, double packed_bytes, bool with_exc, int value_bytes) {
	const double limit = policy_read_ahead_bits(with_exc, value_bytes);
	// (float columns of 1-bit vectors: 0.75 cold, 0.72 with the second stream of reads; double columns of almost nothing but 0-bit vectors — the gov26 shape, a pure stream of
	//  stores: 0.82 with six workgroups per CU and no second stream, 0.71-0.72 with it: kEmptyVectorsBits)
	// (float columns of 1-bit vectors WITH exceptions: 0.44 -> 0.52 with the read-ahead, call 3 — the 1.5-bit floor is for exception-free ones)
	const double least = value_bytes == 8 ? kEmptyVectorsBits : (with_exc ? 0.5 : 1.5);
	return n_vectors >= kReadAheadVectors && packed_bytes <= limit * 128.0 * static_cast<double>(n_vectors) && packed_bytes >= least * 128.0 * static_cast<double>(n_vectors);
}

// The store decode of this column runs with the read-ahead (read_ahead_kernels.hip).  Asked for (1): any column long enough to be worth a second launch whose
// sizes are known (the lead is in vectors per microsecond).  Left to the library (-1, the default): columns of NARROW vectors only — there the decode is bound
// by its two dependent reads under a write-dominated stream (0.68-0.72 of the HBM peak at 2-6 bits, 0.60-0.69 with exceptions) and gains from finding them in
// the Infinity Cache: +3-14 % up to 6 bits (one vector per workgroup), with exceptions +5-24 % up to 7 bits (two per workgroup).  At 7 bits without exceptions
// it is even across six closing runs (-1 %), and an extension to 11 / 9 bits that single-column A/B runs suggested (+2-7 %, call 49) lost 3-6 % in the bench line of
// another box (call 50): the limits are where the gain is robust.  Beyond, the second stream of reads costs more than the hits save (benchmark column 0.77 -> 0.73).
// The lead that goes with a width: policy_read_ahead_pace.  tools/r05_read_ahead*.py, profiles/r05_read_ahead.txt.
// (float columns, round 6: the same kernel beside k_decode_column_f32, limits of their own — above, profiles/r06_float_decode.txt)
__host__ __device__ inline bool policy_read_ahead(const ColumnSizes& s, bool with_exc, int value_bytes, const DecodeOptions& o) {
	if (o.read_ahead == 0 || s.packed_bytes == 0) { return false; }
	if (o.read_ahead > 0) { return s.n_vectors >= kReadAheadForcedVectors; }
	if (o.streams_serialize) { return false; } // (the two kernels cannot run side by side in this process: api_context.hip)
	return policy_read_ahead_auto(s.n_vectors, static_cast<double>(s.packed_bytes), with_exc, value_bytes);
}

// ---- the residency pads of double columns (decode_kernels.hip: launch_decode_column; unused dynamic LDS) ----
// What a CU wants is a certain amount of bytes in flight, not a certain number of workgroups.  One vector per workgroup: eight workgroups per CU up to 33 bits,
// seven up to 35, six beyond; seven for ALP_RD columns.  Two vectors per workgroup: eight / seven / six workgroups by width.  ALPGPU_OPT_DECODE_RESIDENCY_PAD
// overrides (0 = never cap).  (re-measured in round 5 with the per-vector decode loops — a workgroup's stores no longer wait for one another, workgroups live
// shorter and a CU wants somewhat fewer of them: tools/r05_decode_resid.py, profiles/r05_decode_exceptions.txt)
// One vector per workgroup: up to ~30 bits a 6 KiB pad (ten workgroups' worth of LDS for eight: 0.77-0.80 -> 0.79-0.81, with exceptions 0.75-0.79 -> 0.78-0.82 up
// to 38 bits); 30-38 bits without exceptions none; from 38 bits on seven, then six workgroups per CU (+5-7 %); ALP_RD columns — more arithmetic per value — seven.
constexpr int    kPadEightWgsKib  = 6;
constexpr int    kPadSevenWgsKib  = 11;
constexpr int    kPadSixWgsKib    = 14;  // also a pure stream of stores (0-bit vectors): it wants few workgroups per CU, like wide vectors
constexpr double kUncappedBits    = 30.0; // without exceptions no pad from here up to kWideBits
constexpr double kSixWgsBitsExc   = 46.0; // with exceptions seven workgroups per CU from kWideBits, six from here
// Two vectors per workgroup, no exceptions: sixteen vectors in flight per CU up to 8 bits, fourteen (seven workgroups) beyond.  With exceptions the caps lose.
constexpr int    kPadTwoVectorsKib  = 3;
constexpr double kPadTwoVectorsBits = 8.5;

// The host rule for double columns: vectors per workgroup, residency pad and exception stage from the sizes (ahead: what policy_read_ahead said of them).
__host__ __device__ inline DecodeShape policy_shape_f64(const ColumnSizes& s, const DecodeOptions& o, double bits, bool with_exc, bool ahead) {
	DecodeShape sh {(o.forced_vpw == 2 || o.forced_vpw == 4) ? 2 : 1, o.plain_stores, false, o.forced_pad_kib >= 0 ? o.forced_pad_kib : kPadNone, kDecodeStaged, 0};
	if (o.forced_vpw != 0) { return sh; } // (a forced shape is a forced shape)
	const bool hinted     = s.packed_bytes != 0 || s.exc_bytes != 0; // no hints: one vector per workgroup
	const bool mostly_rd  = policy_mostly_rd(static_cast<double>(s.n_vectors), s.rd_vectors);
	const bool auto_ahead = o.read_ahead < 0 && ahead;
	bool       one        = !(hinted && policy_narrow(bits, with_exc));
	// narrow vectors under the read-ahead: their reads hit the Infinity Cache, and ONE vector per workgroup — the shape that suffers most from the two round
	// trips (0.53 at 2-6 bits) — becomes the best one (0.75-0.80); with exceptions two per workgroup stay ahead (0.68-0.74 against 0.64-0.68)
	if (auto_ahead && !with_exc) { one = true; }
	// (almost) nothing but 0-bit vectors — a pure stream of stores, e.g. the gov26 shape: one vector per workgroup (and six workgroups per CU, below): 0.71 -> 0.82 (call 2)
	if (hinted && policy_empty(bits)) { one = true; }
	sh.vectors_per_wg = one ? 1 : 2;
	if (o.forced_pad_kib < 0 && s.packed_bytes != 0 && s.n_vectors != 0 && !auto_ahead) { // (under the read-ahead no cap helps)
		if (one) {
			if (mostly_rd) {
				sh.pad_kib = kPadSevenWgsKib;
			} else if (policy_empty(bits)) {
				sh.pad_kib = kPadSixWgsKib;
			} else if (with_exc) {
				sh.pad_kib = bits >= kSixWgsBitsExc ? kPadSixWgsKib : (policy_wide(bits) ? kPadSevenWgsKib : kPadEightWgsKib);
			} else {
				sh.pad_kib = policy_wide(bits) ? kPadSixWgsKib : (bits >= kUncappedBits ? kPadNone : kPadEightWgsKib);
			}
		} else if (!with_exc && bits > kPadTwoVectorsBits) {
			sh.pad_kib = kPadTwoVectorsKib;
		}
	}
	// exception-heavy columns: the instance with the 256-entry stage (one vector per workgroup, non-temporal stores): 0.72 -> 0.77 on bench.py's 10 %-exceptions column (call 6)
	sh.many_exc = one && !o.plain_stores && s.n_vectors != 0 && static_cast<double>(s.exc_bytes) >= kManyExcBytesPerVector * static_cast<double>(s.n_vectors) && !mostly_rd;
	return sh;
}

// Float columns (round 6): vectors per workgroup — 2 (the bytes in flight of one double vector), FOUR for columns of narrow vectors whose sizes are known, the
// streamed shape where policy_stream_f32 says so, what ALPGPU_OPT_DECODE_VECTORS_PER_WG says otherwise — and the residency pad (ALPGPU_OPT_DECODE_RESIDENCY_PAD,
// else none).  tools/sweep_f32_decode.py, profiles/r06_float_decode.txt.
__host__ __device__ inline DecodeShape policy_shape_f32(const ColumnSizes& s, const DecodeOptions& o, double bits, bool with_exc) {
	int number = o.forced_vpw != 0 ? o.forced_vpw : 2; // (decode_shape_number)
	if (o.forced_vpw == 0 && s.packed_bytes != 0 && s.n_vectors != 0) {
		const double four = with_exc ? kFourVectorsBitsExcF32 : kFourVectorsBitsF32; // (0: never)
		if (four > 0.0 && bits <= four) { number = 4; }
		// narrow vectors without exceptions: streamed by persistent workgroups
		if (policy_stream_f32(s.n_vectors, static_cast<double>(s.packed_bytes), with_exc)) { number = kStreamShapeF32; }
	}
	DecodeShape sh {number, o.plain_stores, false, o.forced_pad_kib >= 0 ? o.forced_pad_kib : kPadNone, kDecodeStaged, 0};
	if (number >= 16) { sh.family = kDecodeStreamed, sh.stream_shape = number; }
	if (number == 8) { sh.family = kDecodeWaveDirect, sh.vectors_per_wg = 4; }
	return sh;
}

// THE host rule: the launch of a column (or a run of one) whose sizes the host knows, and whether the read-ahead runs beside it
struct DecodePlan { DecodeShape shape; bool ahead; };
__host__ __device__ inline DecodePlan policy_decode_plan(const ColumnSizes& s, int value_bytes, const DecodeOptions& o) {
	const bool   with_exc = policy_with_exceptions(static_cast<double>(s.n_vectors), static_cast<double>(s.exc_bytes));
	const double bits     = policy_bits(s.n_vectors, static_cast<double>(s.packed_bytes));
	const bool   ahead    = policy_read_ahead(s, with_exc, value_bytes, o);
	if (value_bytes == 8) { return DecodePlan {policy_shape_f64(s, o, bits, with_exc, ahead), ahead}; }
	const DecodeShape sh = policy_shape_f32(s, o, bits, with_exc);
	return DecodePlan {sh, ahead && sh.family != kDecodeStreamed}; // (a float column streamed by persistent workgroups prefetches for itself; the read-ahead beside it changed nothing: call 14)
}

// The kind of a stretch of vectors, from its sums: adjacent segments of one kind are decoded in one launch (api_decode.hip: plan_decode_runs).  Double columns, by
// packed width: up to the read-ahead's limit / up to the two-vectors-per-workgroup limit / below kWideBits / beyond; float columns: up to the read-ahead's limit /
// up to the four-vectors limit / beyond; each with or without exceptions.
__host__ __device__ inline int policy_stretch_kind(uint64_t n_vectors, uint64_t packed_bytes, uint64_t exc_bytes, int value_bytes) {
	const bool   with_exc = policy_with_exceptions(static_cast<double>(n_vectors), static_cast<double>(exc_bytes));
	const double bits     = policy_bits(n_vectors, static_cast<double>(packed_bytes));
	int          band     = 0;
	if (bits > policy_read_ahead_bits(with_exc, value_bytes)) {
		band = value_bytes == 8 ? (policy_narrow(bits, with_exc) ? 1 : (policy_wide(bits) ? 3 : 2)) : (bits <= (with_exc ? kFourVectorsBitsExcF32 : kFourVectorsBitsF32) ? 1 : 2);
	}
	return 2 * band + (with_exc ? 1 : 0);
}

// The read-ahead's pace and lead.  The lead is a TIME: what the read-ahead brings into the Infinity Cache stays there for some tens of microseconds only (the
// decode's own stores stream through it) and has to be there before the decode asks.  In vectors: that time at the rate of a decode running at 0.78 of the full
// HBM bandwidth.  How long: by the vectors' width unless set — best leads measured per width: 15 / 20 / 30 / 30 / 35 / 40 / 50 us at 1 .. 7 bits, 50-70 us at
// 8-11, with and without exceptions; too short falls off a cliff whose place moves a little from box to box, too long decays slowly: a little above the optimum,
// 12 + 6.5 us per bit, at most 60 (profiles/r05_read_ahead.txt).  The read-ahead itself stretches the lead when its batches arrive late (read_ahead_kernels.hip).
struct ReadAheadPace {
	uint32_t lead_min, lead_max, ps_per_vector;
};
__host__ __device__ inline ReadAheadPace policy_read_ahead_pace(double n_vectors, double packed_bytes, double exc_bytes, int value_bytes, int lead_us_option) {
	const double out_bytes = 1024.0 * value_bytes;
	const double per_vec   = (packed_bytes + exc_bytes) / n_vectors + 32.0;
	const double ps_vec    = (out_bytes + per_vec) / 8.0; // picoseconds per vector at 8 TB/s: an upper bound of the decode's rate (the read-ahead's naps by it never overshoot)
	const double bits      = packed_bytes / (128.0 * n_vectors);
	const double by_width  = value_bytes == 8 ? 12.0 + 6.5 * bits : 12.0 + 3.0 * bits; // (float columns: ~20 us at 3-6 bits, call 1b)
	const double lead_us   = lead_us_option > 0 ? static_cast<double>(lead_us_option) : (by_width > 60.0 ? 60.0 : by_width);
	const double lead      = lead_us * 1.0e6 / ps_vec * 0.78;
	ReadAheadPace p;
	p.lead_max      = static_cast<uint32_t>(lead < 4096.0 ? 4096.0 : (lead > 4.0e9 ? 4.0e9 : lead));
	p.lead_min      = 2048; // about what is resident when a workgroup reports: those vectors' reads are under way
	p.ps_per_vector = static_cast<uint32_t>(ps_vec);
	return p;
}

// ---- the unhinted decode's candidate launches (api_decode.hip: decode_unhinted launches one or all of them; k_unhinted_plan says which one runs) ----
// A deliberate coarsening of the host rule to three shapes for double columns and one for float columns (four never pay, see above): the plan word holds the
// candidate's number, 1-based (0 in a launch's gate: not a candidate).
enum UnhintedCandidateF64 : int { kUnhintedOneVector = 1, kUnhintedTwoVectors = 2, kUnhintedSevenWgs = 3 };
constexpr int kUnhintedShapesF64 = 3;
constexpr int kUnhintedShapesF32 = 1;
constexpr DecodeShape kUnhintedCandidatesF64[kUnhintedShapesF64] = {
	{1, false, false, kPadEightWgsKib, kDecodeStaged, 0}, // kUnhintedOneVector: up to ~38 bits — and the shape a column without hints always got
	{2, false, false, kPadNone, kDecodeStaged, 0},        // kUnhintedTwoVectors: narrow vectors
	{1, false, false, kPadSevenWgsKib, kDecodeStaged, 0}, // kUnhintedSevenWgs: vectors of 38 bits and more, ALP_RD columns, 0-bit vectors
};
constexpr DecodeShape kUnhintedCandidatesF32[kUnhintedShapesF32] = {{2, false, false, kPadNone, kDecodeStaged, 0}};
struct UnhintedChoice { int shape; bool ahead; }; // (shape: 1-based)
__host__ __device__ inline UnhintedChoice policy_unhinted(uint64_t n_vectors, double packed_bytes, double exceptions, double rd_vectors, int value_bytes, int read_ahead_option) {
	const double n         = static_cast<double>(n_vectors);
	const double exc_bytes = (value_bytes + 2.0) * exceptions;
	const bool   with_exc  = policy_with_exceptions(n, exc_bytes);
	const double bits      = packed_bytes / (128.0 * n);
	UnhintedChoice c;
	c.ahead = read_ahead_option > 0 ? n_vectors >= kReadAheadForcedVectors : (read_ahead_option < 0 && policy_read_ahead_auto(n_vectors, packed_bytes, with_exc, value_bytes));
	if (value_bytes == 8) {
		const bool narrow = policy_narrow(bits, with_exc) && !policy_empty(bits);
		const bool seven  = policy_mostly_rd(n, rd_vectors) || policy_wide(bits) || policy_empty(bits);
		c.shape           = narrow ? kUnhintedTwoVectors : (seven ? kUnhintedSevenWgs : kUnhintedOneVector);
		if (read_ahead_option < 0 && c.ahead && !with_exc) { c.shape = kUnhintedOneVector; } // under the read-ahead one vector per workgroup is the best shape without exceptions
	} else {
		c.shape = 1;
	}
	return c;
}

} // namespace alpgpu
