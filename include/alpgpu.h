/*
 * alpgpu.h — C ABI of libalpgpu.so: the MI355X (gfx950) ALP / ALP_RD vector codec.
 *
 * This is the drop-in boundary of the repository.  Everything behind it is hand-written HIP for CDNA4;
 * there is NO CPU fallback: every entry point fails with ALPGPU_ERR_NO_DEVICE when no gfx950 device is
 * usable.  The C++ header include/alp.hpp (source-compatible with the reference's include/alp.hpp:4-13)
 * and the Python harness (alp_amd/capi.py) are both thin callers of these functions.
 *
 * The reference (cwida/ALP) has no FFI layer; its boundary is the C++ vector API.  Each batch entry
 * point below names the reference function(s) it replaces, file:line relative to /root/reference:
 *
 *   alpgpu_rowgroup_init_f64   alp::encoder<double>::init            include/alp/encoder.hpp:420-427
 *                              (sampler::first_level_sample           include/alp/sampler.hpp:14-52,
 *                               find_top_k_combinations               include/alp/encoder.hpp:139-235)
 *                              alp::rd_encoder<double>::init          include/alp/rd.hpp:180-185 (:33-104)
 *   alpgpu_state_from_samples_f64  find_top_k_combinations (:139-235) + find_best_dictionary (rd.hpp:89-104) on given samples
 *   alpgpu_encode_f64          alp::encoder<double>::encode           include/alp/encoder.hpp:402-418
 *                              (find_best_exponent_factor_from_combinations :241-305, encode_simdized :307-400)
 *                              alp::encoder<double>::analyze_ffor     include/alp/encoder.hpp:109-120
 *                              ffor::ffor(int64/uint64/uint16)        include/fastlanes/ffor.hpp:7-15
 *                                                                     (src/fastlanes_generated_ffor.cpp:29781,29939)
 *                              alp::rd_encoder<double>::encode        include/alp/rd.hpp:109-147
 *   alpgpu_decode_f64          generated::falp::fallback::scalar::falp include/alp/falp.hpp:10-26 (src/falp.cpp:42440)
 *                              alp::decoder<double>::patch_exceptions include/alp/decoder.hpp:141-149
 *                              unffor::unffor(uint64/uint16)          include/fastlanes/unffor.hpp:7-15
 *                              alp::rd_encoder<double>::decode        include/alp/rd.hpp:152-178
 *   alpgpu_decode_sum_f64      falp + patch_exceptions fused with a SUM consumer (bench_end_to_end .../queries/q1.cpp:63-104)
 *   alpgpu_ffor_i64 / alpgpu_unffor_i64 / alpgpu_ffor_u16 / alpgpu_unffor_u16 / alpgpu_ffor_u8 / alpgpu_unffor_u8 (+ _i32, float section)
 *                              ffor::ffor / unffor::unffor            include/fastlanes/{ffor,unffor}.hpp:7-15
 *   alpgpu_falp_f64            falp (no exception patching)           include/alp/falp.hpp:10-26
 *   alpgpu_decode_values_f64   alp::decoder<double>::decode           include/alp/decoder.hpp:134-138
 *   alpgpu_patch_f64           alp::decoder<double>::patch_exceptions include/alp/decoder.hpp:141-149
 *   alpgpu_encode_simdized_f64 alp::encoder<double>::encode_simdized  include/alp/encoder.hpp:307-400
 *   alpgpu_analyze_ffor_i64    alp::encoder<double>::analyze_ffor     include/alp/encoder.hpp:109-120
 *   alpgpu_rd_encode_vectors_f64 / alpgpu_rd_decode_vectors_f64
 *                              alp::rd_encoder<double>::encode/decode include/alp/rd.hpp:109-147 / :152-178
 *
 * Conventions
 *   - plain C types; every pointer named d_* is a DEVICE pointer (HBM) unless stated otherwise;
 *   - a "vector" is 1024 values, a "rowgroup" is 100 vectors (reference include/alp/config.hpp:11-15);
 *     rowgroup r owns vectors 100r .. 100r+99 and one state (scheme, (e,f) candidates / RD dictionary);
 *   - all work is enqueued on the context's stream (alpgpu_set_stream) and is asynchronous; call
 *     alpgpu_synchronize (or synchronise the stream yourself) before reading results on the host;
 *   - return value: ALPGPU_OK or a negative ALPGPU_ERR_*; alpgpu_last_error() gives the text (thread-local);
 *   - no C++ exceptions cross this boundary; one context per device, used by one host thread at a time.
 */
#ifndef ALPGPU_H
#define ALPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALPGPU_VECTOR_SIZE 1024u
#define ALPGPU_ROWGROUP_VECTORS 100u
#define ALPGPU_MAX_COMBINATIONS 5u
#define ALPGPU_RD_DICT_SIZE 8u

/* same numeric values as the reference's alp::Scheme (include/alp/constants.hpp:10-14) */
#define ALPGPU_SCHEME_INVALID 0u
#define ALPGPU_SCHEME_ALP_RD 1u
#define ALPGPU_SCHEME_ALP 2u

#define ALPGPU_OK 0
#define ALPGPU_ERR_NO_DEVICE (-1)   /* no usable gfx950 device / HIP runtime failure at start-up */
#define ALPGPU_ERR_INVALID (-2)     /* bad argument */
#define ALPGPU_ERR_HIP (-3)         /* a HIP call failed; see alpgpu_last_error() */
#define ALPGPU_ERR_CAPACITY (-4)    /* an output stream was too small (reported by alpgpu_column_totals) */

typedef struct alpgpu_ctx alpgpu_ctx;

/* Per-rowgroup codec state in HBM (32 bytes).  Mirror of the fields of alp::state<double>
 * (reference include/alp/encoder.hpp:35-62) that outlive init(). */
typedef struct alpgpu_rowgroup_state {
	uint8_t  scheme;      /* ALPGPU_SCHEME_ALP | ALPGPU_SCHEME_ALP_RD */
	uint8_t  k;           /* ALP: number of (e,f) candidates, 1..5 (state.k_combinations) */
	uint8_t  combos[10];  /* ALP: combos[2i] = exponent e, combos[2i+1] = factor f (best_k_combinations) */
	uint8_t  rd_rbw;      /* ALP_RD: right_bit_width (48..63) */
	uint8_t  rd_lbw;      /* ALP_RD: left_bit_width (1..3) */
	uint8_t  rd_dict_size;/* ALP_RD: actual_dictionary_size (1..8) */
	uint8_t  pad;
	uint16_t rd_dict[8];  /* ALP_RD: left_parts_dict */
} alpgpu_rowgroup_state;

/* Per-vector descriptor in HBM (32 bytes, 32-byte aligned; one scalar load per wavefront).
 * Modelled on the reference's per-vector metadata (state.exp/fac/bit_width/for_base + exceptions_count;
 * the 48-byte alp_m record of publication/source_code/bench_end_to_end/include/encoding/helper.hpp:36-67). */
typedef struct alpgpu_vector_desc {
	uint64_t packed_off;  /* byte offset of this vector's bit-packed words in the packed stream (multiple of 128).
	                         ALP: 128*bw bytes.  ALP_RD: 128*rbw bytes (right, u64 lanes) then 128*lbw (left, u16 lanes) */
	uint64_t exc_off;     /* byte offset of this vector's exception record in the exception stream (multiple of 8).
	                         ALP: cnt*8 B values (f64 bits) then cnt*2 B positions.  ALP_RD: cnt*2 B left parts then cnt*2 B positions.
	                         record size is rounded up to 8 bytes; both encode forms write the pad bytes as zero (the streams are byte-reproducible into a dirty buffer) */
	int64_t  base;        /* ALP: frame-of-reference base (for_base).  ALP_RD: 0 */
	uint8_t  bw;          /* ALP: bit width 0..64.  ALP_RD: right bit width */
	uint8_t  e;           /* ALP: exponent index (state.exp) */
	uint8_t  f;           /* ALP: factor index (state.fac) */
	uint8_t  lbw;         /* ALP_RD: left bit width; ALP: 0 */
	uint16_t exc_cnt;     /* number of exceptions 0..1024 */
	uint16_t scheme;      /* copy of the rowgroup's scheme */
} alpgpu_vector_desc;

/* A compressed column resident in HBM.  All buffers are caller-allocated (alpgpu_malloc or any HIP
 * allocator, e.g. a torch tensor) and caller-owned, like every buffer of the reference API. */
typedef struct alpgpu_column {
	uint64_t               n_vectors;
	uint64_t               n_rowgroups;     /* ceil(n_vectors / 100) */
	alpgpu_rowgroup_state* d_rowgroups;     /* [n_rowgroups] */
	alpgpu_vector_desc*    d_vectors;       /* [n_vectors] */
	uint8_t*               d_packed;        /* packed stream, 128-byte aligned */
	uint64_t               packed_capacity; /* bytes; worst case n_vectors * 8448 */
	uint8_t*               d_exc;           /* exception stream, 8-byte aligned */
	uint64_t               exc_capacity;    /* bytes; worst case n_vectors * 10240 */
	uint64_t*              d_totals;        /* [8]: [0] packed bytes used, [1] exception bytes used, [2] overflow flag, [3] look-back stall flag of the
	                                           single-pass encode (always 0 once alpgpu_encode_* has drained: the recovery route clears it),
	                                           [4..5] running totals of the encode launch in flight, [6] recovery gate (latched from [3]),
	                                           [7] ALP_RD rowgroups as last counted by alpgpu_column_totals */
	/* host-side hints (0 = unknown): stream sizes as last seen by the host.  Filled by alpgpu_column_totals and
	 * alpgpu_column_from_blob; decode uses them only to pick its launch shape (ALPGPU_OPT_DECODE_VECTORS_PER_WG = 0 "auto") */
	uint64_t               packed_bytes_hint;
	uint64_t               exc_bytes_hint;
	/* optional (NULL = absent; ABI version 2), ALP_RD rowgroups only: ALPGPU_RD_ORDER_STRIDE u16 words per rowgroup =
	 * { D, then the D distinct sampled left parts in the reference's sorted order (left_parts_sorted_repetitions,
	 * include/alp/rd.hpp:47-60) }.  alpgpu_rowgroup_init_* writes it; alpgpu_encode_vectors_* reads it to pack, at exception
	 * slots, the left index the reference packs there (its map position, rd.hpp:69-77, :130-135).  Without it those slots
	 * carry the dictionary size.  No decoder reads these bits; a table that does not start with the rowgroup's dictionary
	 * (e.g. states supplied by the caller) is ignored. */
	uint16_t*              d_rd_order;
	/* host-side hint (ABI version 3; zero-initialise it): 0 = unknown, else 1 + the number of ALP_RD rowgroups of the column, as counted by
	 * alpgpu_column_totals (a small kernel over d_rowgroups) or alpgpu_column_from_blob.  Informational: the fused consumers chose their
	 * kernel by it while the one-wavefront kernel's ALP_RD arm spilled; they no longer read it. */
	uint64_t               alp_rd_rowgroups_hint;
} alpgpu_column;
#define ALPGPU_RD_ORDER_STRIDE 296u

/* ---- context / plumbing ------------------------------------------------------------------------- */
int         alpgpu_ctx_create(int device, alpgpu_ctx** out_ctx);
int         alpgpu_init(int device, alpgpu_ctx** out_ctx); /* the name SURVEY.md §8(b) uses for the same call */
void        alpgpu_ctx_destroy(alpgpu_ctx* ctx);
const char* alpgpu_last_error(void);
int         alpgpu_abi_version(void);
/* run on a caller-provided hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = the device's
 * default (null) stream.  A new context runs on its own non-blocking stream until this is called. */
int         alpgpu_set_stream(alpgpu_ctx* ctx, void* hip_stream);
int         alpgpu_use_own_stream(alpgpu_ctx* ctx);
int         alpgpu_synchronize(alpgpu_ctx* ctx);
/* tuning knobs (never change results).  ALPGPU_OPT_DECODE_VECTORS_PER_WG: 1 or 2 consecutive vectors per decode
 * workgroup, or 0 (default) = choose from the column's size hints: 2 keeps twice the bytes in flight and is faster for
 * narrow columns (average packed width <= 17 bits; <= 22 bits when there are about two or more exceptions per vector: crossovers
 * re-measured at one-bit resolution in rounds 4 and 5), 1 for wider ones — every ALP_RD column.  A column without size hints: ALPGPU_OPT_DECODE_UNHINTED.
 * Float columns: 1, 2 or 4; 8 = one wavefront per vector; 16..30 = the column STREAMED by persistent workgroups (decode_stream_f32_kernels.hip: loading
 * wavefronts several chunks ahead, decoding wavefronts that own whole vectors; the values name chunk size / arena / wavefront counts, 27 = chunks of 12 vectors,
 * 24 KiB of records per chunk, 12 decoding + 2 loading wavefronts, one workgroup per CU).  0 = 2, and 27 for hinted columns of >= 32 768 vectors with more
 * than 1.5 and at most 8.5 packed bits per value and fewer than ~2 exceptions per vector (round 6: 0.65-0.72 of the HBM peak against 0.60-0.62).
 * Double columns run 4 as 2 (round 4's four-vectors-per-workgroup shape lost at every width and is gone: profiles/r04_decode_floor.txt).
 * ALPGPU_OPT_DECODE_PLAIN_STORES: 1 = ordinary instead of non-temporal stores. */
#define ALPGPU_OPT_DECODE_VECTORS_PER_WG 1
#define ALPGPU_OPT_DECODE_PLAIN_STORES 2
/* ALPGPU_OPT_ENCODE_TWO_PASS: 1 = analysis pass + scan + pack pass (reads the input twice) instead of the default
 * single-pass encode whose output offsets come from an in-kernel look-back; both give byte-identical columns, double and
 * float.  The single pass needs its predecessor workgroups to run; should its look-back ever give up (HIP promises no
 * dispatch order), the two-pass kernels enqueued behind it on the same stream redo the column: callers see a complete column. */
#define ALPGPU_OPT_ENCODE_TWO_PASS 3
/* ALPGPU_OPT_DEBUG_FORCE_STALL: 1 = every look-back of the single pass that has to wait gives up at once (tests of the
 * recovery route; the result is still a complete, byte-identical column). */
#define ALPGPU_OPT_DEBUG_FORCE_STALL 4
/* ALPGPU_OPT_ENCODE_ASYNC_INIT: 1 (default) = alpgpu_encode_f64 of a column of >= 1024 rowgroups runs the rowgroup search as a
 * persistent kernel on a second, internal stream BESIDE the single-pass vector encode, which polls for each rowgroup's state (the two
 * rejoin the context's stream before the call's last launches: callers still see one stream); 0 = search, then vectors, on one stream;
 * 2 = beside the encode for float columns as well (measured slower there: the float tiles leave the search no room).  Results are
 * identical in every mode. */
#define ALPGPU_OPT_ENCODE_ASYNC_INIT 6
/* ALPGPU_OPT_CONSUMER_PIPELINED: which kernel runs alpgpu_decode_sum_f64 / alpgpu_decode_count_range_f64 / alpgpu_column_sum_f64.
 * 0 (default) and 2 = ONE wavefront per vector (no barrier, one wave-uniform prologue per vector, eight wavefronts per SIMD), whatever the
 *     column holds: narrow ALP vectors (bit width <= 28, <= 48 exceptions) staged whole in the wavefront's LDS by LDS-DMA, every other
 *     vector's packed words read straight from HBM with bounded buffer loads;
 * 3 = the staged kernel (four wavefronts per vector, one short-lived workgroup per two vectors); same bits as 0 / 2 (the order documented
 *     at alpgpu_decode_sum_f64);
 * 1 = the persistent, software-pipelined kernel of alp_amd/csrc/consume_kernels.hip (one wavefront per vector, packed words, exception
 *     records and descriptors prefetched into per-wavefront LDS rings by LDS-DMA).  Its summation order is its own: lane L adds its 16
 *     values 128m + 2L, 128m + 2L + 1 (m = 0..7) in ascending order from +0.0, then the adjacent-lane tree over the 64 lane sums.
 * Measured in round 3 (profiles/r03_consumers.txt): what the staged kernel runs out of is instruction issue, the scalar unit first; the
 * one-wavefront kernel does a quarter of its scalar work per vector and is 7-30 % faster on ALP and ALP_RD columns alike (while its ALP_RD
 * arm still spilled, the default chose between the two by alpgpu_column::alp_rd_rowgroups_hint); the ring kernel is slower than both. */
#define ALPGPU_OPT_CONSUMER_PIPELINED 5
/* Retired options: alpgpu_set_option accepts the values it always accepted and they have no effect (the variants they selected lost and are gone).
 * ALPGPU_OPT_ENCODE_KERNEL (ALPGPU_ENCODE_KERNEL_LEAN / _CLASSIC): the single-pass double encode is always the lean kernel.
 * ALPGPU_OPT_DECODE_PAIRING (0..3): workgroups that owned two vectors and chose from their descriptors how to run them.
 * ALPGPU_OPT_DECODE_PATCH_AFTER (0..64): exceptions patched in after the stores (profiles/r05_decode_exceptions.txt). */
#define ALPGPU_OPT_ENCODE_KERNEL 7
#define ALPGPU_ENCODE_KERNEL_LEAN 0
#define ALPGPU_ENCODE_KERNEL_CLASSIC 1
#define ALPGPU_OPT_DECODE_PAIRING 8
#define ALPGPU_OPT_DECODE_PATCH_AFTER 9
/* ALPGPU_OPT_ENCODE_UNORDERED (double and float columns; round 5; default 0): 1 = alpgpu_encode_* / alpgpu_encode_vectors_* do not
 * assign stream offsets in vector order.  Each 8-vector tile reserves its packed / exception bytes with ONE atomic add when its analysis is done,
 * instead of waiting for the sizes of every tile before it (the ordered form's look-back).  Every vector's record — descriptor fields, packed words,
 * exception values and positions — is byte for byte what the ordered form writes; what changes is WHERE in d_packed / d_exc a tile's records lie
 * (tiles in the order they finished; the eight vectors of a tile stay adjacent, in order), so the two streams as a whole are a permutation of
 * the reference's by tiles and differ from run to run.  Every decoder and consumer of this library follows the descriptors' offsets and
 * does not care; alpgpu_column_to_blob serializes such a column as it is (alpgpu_column_from_blob's validation accepts it: records may lie
 * anywhere inside the streams as long as they do not leave them); alpgpu_decompress_host_* — which uploads a blob's streams chunk by chunk and relies on
 * offsets that ascend with the vector index — refuses such a blob (ALPGPU_ERR_INVALID): decode it with alpgpu_column_from_blob + alpgpu_decode_*.
 * The host pipeline (alpgpu_compress_host_*) always uses the ordered form.
 * If the rowgroup search beside the encode stalls, the recovery route rewrites the column in vector order. */
#define ALPGPU_OPT_ENCODE_UNORDERED 10
/* ALPGPU_OPT_DECODE_RESIDENCY_PAD (tuning aid): KiB of unused dynamic LDS every double store-decode workgroup asks for, which caps the workgroups
 * resident per CU (160 KiB / (its own 9.6 or 19.3 KiB + this)); -1 (default) = chosen from the column's size hints (what a CU wants
 * is an amount of bytes in flight).  Never changes results (tests/test_decode_gpu.py: 0 .. 120 KiB at one and two vectors per workgroup); a pad that does not fit
 * beside the workgroup's own LDS any more (150 KiB with two vectors per workgroup) makes the launch fail: alpgpu_decode_f64 returns ALPGPU_ERR_HIP, nothing is written. */
#define ALPGPU_OPT_DECODE_RESIDENCY_PAD 11
/* ALPGPU_OPT_DECODE_READ_AHEAD (store decode, double since round 5, float since round 6): alpgpu_decode_f64 / _f32 start a READ-AHEAD beside the decode kernel — a few persistent workgroups
 * on the context's second stream that pull descriptors, packed words and exception records into the Infinity Cache ALPGPU_OPT_DECODE_READ_AHEAD_US
 * microseconds (default 0 = by the vectors' width: 18 us at 1 bit .. 60 us from 8 bits on) ahead of the decode kernel, which tells them where it is; the decode's two dependent reads then hit the cache.
 *   -1 (default)  columns of >= 262144 vectors of at most 6 packed bits per value on average (7 when they have exceptions) whose size hints are set (+3-24 % there; wider columns lose);
 *    0            never;   1  every column of >= 32768 vectors whose size hints are set (measurements).
 * Same output bytes.  The two kernels are joined on the context's stream: work enqueued behind alpgpu_decode_f64 waits for both.
 * Where kernels of two streams cannot run side by side (GPU_MAX_HW_QUEUES=1, AMD_SERIALIZE_KERNEL, HIP_LAUNCH_BLOCKING, a counter-collection pass) the read-ahead
 * leaves when no word from the decode arrives (round 6: within max(200 us, a quarter of the decode's own estimated duration); until round 5 a flat 50 ms), and a context
 * created with one of those three variables set does not start it on its own (-1 behaves as 0).  One context runs ONE store decode at a time (one progress word). */
#define ALPGPU_OPT_DECODE_READ_AHEAD 12
#define ALPGPU_OPT_DECODE_READ_AHEAD_US 13
/* ALPGPU_OPT_DECODE_SEGMENTS (double store decode; round 5; default 1): alpgpu_column_totals and alpgpu_column_from_blob remember, in the context, the sizes of up to 32
 * segments of the column; alpgpu_decode_f64 of that column through the same context merges adjacent segments of the same kind (by packed width and exceptions) into at most 8 runs
 * and decodes run by run, each with the launch shape (and read-ahead) its own sizes call for — a column whose regions differ is no longer decoded in the shape of its average.
 * Columns of one kind, columns without the call, forced launch shapes: one launch, as before.  0 = never.  alpgpu_decode_runs tells.  Same bytes. */
#define ALPGPU_OPT_DECODE_SEGMENTS 14
/* ALPGPU_OPT_DECODE_UNHINTED (round 6; default 1): a column of >= 65536 vectors whose packed_bytes_hint and exc_bytes_hint are both 0 — encoded a moment ago, nobody called
 * alpgpu_column_totals (a host synchronisation) — no longer decodes blind: its sizes are summed on the stream and the launch rule is evaluated on the DEVICE.
 *   1  the decode kernel is launched in the shape such a column always got (one vector per workgroup; float: two) and the read-ahead beside it takes "whether", its lead
 *      and its pace from the device-side plan (long narrow columns: 0.50 -> 0.60 of the HBM peak on the first decode); the sums travel to page-locked host memory behind an
 *      event that is only queried, and the next alpgpu_decode_* of the same column (same buffers and length, not encoded again through this context in between) is planned
 *      on the host like a hinted one — shape, residency, regions (0.72-0.76);
 *   2  as 1, and the first decode launches EVERY candidate shape gated on the plan's word (closed candidates cost their dispatch: ~0.19 ms per 1 Mi empty workgroups,
 *      which is why this is not the default: profiles/r06_decode_policy.txt);
 *   0  one vector per workgroup (float: two), no read-ahead, nothing learned: as before round 6.
 * No host synchronisation in any mode.  Same bytes. */
#define ALPGPU_OPT_DECODE_UNHINTED 15
int         alpgpu_set_option(alpgpu_ctx* ctx, int option, int64_t value);
/* the launch shape alpgpu_decode_f64 (is_f32 = 0) or alpgpu_decode_f32 (1) would use for this column now: vectors per decode
 * workgroup — double: 1 or 2; float: 1, 2, 4 or 8, or 16..30 for the streamed shapes — from ALPGPU_OPT_DECODE_VECTORS_PER_WG and the column's size hints;
 * negative on bad arguments */
int         alpgpu_decode_vectors_per_wg(alpgpu_ctx* ctx, const alpgpu_column* col, int is_f32);
/* ... and whether that decode would run with the read-ahead beside it (ALPGPU_OPT_DECODE_READ_AHEAD): 1 / 0; negative on bad arguments */
int         alpgpu_decode_reads_ahead(alpgpu_ctx* ctx, const alpgpu_column* col, int is_f32);
/* ... and in how many launches alpgpu_decode_f64 (alpgpu_decode_runs_f32: alpgpu_decode_f32) would decode it (ALPGPU_OPT_DECODE_SEGMENTS): 1, or the number of runs; negative
 * on bad arguments.  The three functions above describe the plan of a column whose sizes the host knows, for the column as a WHOLE: a column decoded in several runs gets
 * a shape per run (alpgpu_decode_runs > 1), an unhinted one the shape its device-side plan picks (alpgpu_debug_unhinted_plan). */
int         alpgpu_decode_runs(alpgpu_ctx* ctx, const alpgpu_column* col);
int         alpgpu_decode_runs_f32(alpgpu_ctx* ctx, const alpgpu_column* col);
/* debug aids (tests; both wait for the context's streams): batches of 64 vectors this context's read-aheads have read since it was created; and the plan of its last
 * unhinted decode: out6[0] the candidate that ran (double: 1 = one vector per workgroup, 2 = two, 3 = one with seven workgroups per CU; float: 1 = two, 2 = four),
 * [1] read-ahead lead_min | lead_max << 32 in vectors (0: none), [2] picoseconds per vector | widest record read ahead << 32, [3..5] packed bytes, exceptions, ALP_RD vectors */
int         alpgpu_debug_read_ahead_batches(alpgpu_ctx* ctx, uint64_t* batches);
int         alpgpu_debug_unhinted_plan(alpgpu_ctx* ctx, uint64_t* out6);
/* ... and: forget what the context remembers about this column (its segments, what an unhinted decode learned), as every alpgpu_encode_* into it does */
int         alpgpu_debug_forget_column(alpgpu_ctx* ctx, const alpgpu_column* col);
/* ... and: the launch alpgpu_decode_f64 (is_f32 = 0) / _f32 (1) would make for this column now, as a whole (without a region plan; waits for nothing): out4[0] the
 * double variant word (bit 0: one vector per workgroup, bit 1: plain stores, bit 6: the 256-entry exception stage, bits 8..: residency pad in KiB) or the float shape
 * word (bits 0-7: vectors per workgroup or streamed shape, bits 8..: pad in KiB, 0xFF none), out4[1..3] the packed bytes, exception bytes and ALP_RD rowgroups + 1 it is
 * planned from (for an unhinted column: what an earlier decode of it learned).  Returns 1 (planned on the host), 0 (an unhinted decode, planned on the device;
 * out4 untouched) or negative on bad arguments. */
int         alpgpu_debug_decode_plan(alpgpu_ctx* ctx, const alpgpu_column* col, int is_f32, uint64_t* out4);
/* ---- host-resident columns -----------------------------------------------------------------------------------------------
 * The reference's callers (publication/source_code/bench_compression_ratio/alp.cpp:198-229) hold the column and what they
 * compress it into in host memory.  These entry points take it from there: n_values values at h_in (the last vector may be
 * incomplete: it is padded as alpgpu_pad_tail_* does) become a serialized column at h_blob — byte for byte the blob that
 * alpgpu_encode_* + alpgpu_column_to_blob produce for the same values — and back.  Inside, chunks of whole rowgroups travel up on
 * one stream while the previous chunk is encoded on another and its packed bytes come down; the exception stream collects in HBM and follows at the end
 * (decompression: streams up chunk by chunk, each chunk decoded from a view of the column, doubles down on the chunk's stream).
 * Page-locked h_in / h_blob / h_out (alpgpu_malloc_host) give the link's rate (measured host to host: ~40 GB/s of doubles each
 * way); pageable memory works, at the runtime's staging rate.  Synchronous: everything has arrived when the call returns.
 * Capacity: alpgpu_blob_size(n_vectors, alpgpu_packed_capacity(n_vectors), alpgpu_exc_capacity(n_vectors)) always suffices; a
 * smaller buffer returns ALPGPU_ERR_CAPACITY with the needed size in *written.  The context's stream is left as it was. */
int alpgpu_compress_host_f64(alpgpu_ctx* ctx, const double* h_in, uint64_t n_values, void* h_blob, uint64_t capacity, uint64_t* written);
int alpgpu_compress_host_f32(alpgpu_ctx* ctx, const float* h_in, uint64_t n_values, void* h_blob, uint64_t capacity, uint64_t* written);
/* *n_values receives the column's value count (also when h_out is too small: ALPGPU_ERR_CAPACITY); the blob is validated first */
int alpgpu_decompress_host_f64(alpgpu_ctx* ctx, const void* h_blob, uint64_t size, double* h_out, uint64_t out_capacity_values, uint64_t* n_values);
int alpgpu_decompress_host_f32(alpgpu_ctx* ctx, const void* h_blob, uint64_t size, float* h_out, uint64_t out_capacity_values, uint64_t* n_values);

/* The same over SEVERAL contexts — normally one per GPU of the node, each with its own PCIe link (several contexts on one device work
 * too): the column is cut into n_ctx contiguous whole-rowgroup shards (sizes differ by at most one rowgroup, the rule of
 * alp_amd/sharding.py: rowgroup_shard), shard i runs through ctxs[i]'s pipeline on its own host thread, and the pieces become ONE blob —
 * byte for byte the blob alpgpu_compress_host_* writes with a single context (the descriptors' stream offsets continue where the
 * shards before ended: no collective, a host-side concatenation is the only exchange).  This is how a C / C++ caller that holds a
 * host column (publication/source_code/bench_compression_ratio/alp.cpp:198-229; the worker loop of
 * publication/source_code/bench_end_to_end/src/benchmarks/alp/run_query.cpp:233-305) uses all GPUs of a node from one process.
 * Capacity: regions of the caller's buffer, proportional to the shards' vector counts, serve as the shards' staging, so a shard that
 * compresses worse than the column's average can fail with ALPGPU_ERR_CAPACITY although the sum would fit; *written is then the capacity with
 * which every shard fits its region (never more than the worst-case size alpgpu_blob_size(n, packed_capacity(n), exc_capacity(n)), which
 * always suffices — the capacities' constant terms cover the regions' 8-byte rounding for n_ctx <= 64); on success *written is the blob's size.
 * A context must not be used by anything else during the call; ctxs[i] must be distinct. */
int alpgpu_compress_host_multi_f64(alpgpu_ctx* const* ctxs, int n_ctx, const double* h_in, uint64_t n_values, void* h_blob, uint64_t capacity, uint64_t* written);
int alpgpu_compress_host_multi_f32(alpgpu_ctx* const* ctxs, int n_ctx, const float* h_in, uint64_t n_values, void* h_blob, uint64_t capacity, uint64_t* written);
int alpgpu_decompress_host_multi_f64(alpgpu_ctx* const* ctxs, int n_ctx, const void* h_blob, uint64_t size, double* h_out, uint64_t out_capacity_values,
                                     uint64_t* n_values);
int alpgpu_decompress_host_multi_f32(alpgpu_ctx* const* ctxs, int n_ctx, const void* h_blob, uint64_t size, float* h_out, uint64_t out_capacity_values,
                                     uint64_t* n_values);

/* Measurement aid, not part of the codec: launches the memory traffic of the single-pass encode without its arithmetic — the same
 * launch shape, every 8 KiB vector of d_in read once, write_bytes_per_vector (a multiple of 16, <= 8192) written per vector at
 * d_out + v * write_bytes_per_vector, stored data depending on all loaded data.  bench.py times it to put a measured ceiling for the
 * encode's read/write mix next to the nominal HBM peak. */
int         alpgpu_debug_traffic_probe(alpgpu_ctx* ctx, const void* d_in, void* d_out, uint64_t n_vectors, uint32_t write_bytes_per_vector);
/* ... and with the rowgroup search of alpgpu_encode_f64 (the search of /root/reference include/alp/encoder.hpp:139-235 and rd.hpp:89-104, over d_in, a column
 * of doubles) running beside it on the context's second stream, launched exactly as the encode launches it; its states go to scratch->d_rowgroups
 * (and d_rd_order).  n_vectors >= 102400 (the search runs beside the encode from 1024 rowgroups on).  write_bytes_per_vector = 0 makes either probe a
 * read-only stream of the input.  Round 5: the measured speed of light of "the encode's bytes + the search's instructions" for bench.py. */
int         alpgpu_debug_traffic_probe_with_search(alpgpu_ctx* ctx, const double* d_in, void* d_out, uint64_t n_vectors, uint32_t write_bytes_per_vector,
                                                   alpgpu_column* scratch);
/* Measurement aid, not part of the codec: alpgpu_decode_sum_f64 with the unpack arithmetic left out — the same descriptor and packed-word
 * loads into LDS, the same barrier and reduction, one double per vector written to d_out (its value means nothing).  bench.py times it
 * to say how much of the fused consumers' time is their chain of dependent loads. */
int         alpgpu_debug_decode_probe_f64(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_out);
/* device properties the bench reports: [0]=CU count, [1]=LDS bytes/CU... see alp_amd/capi.py */
int         alpgpu_device_info(alpgpu_ctx* ctx, char* name_out, size_t name_cap, int* cu_count, uint64_t* hbm_bytes);

/* device memory helpers for hosts that do not link a HIP runtime themselves (include/alp.hpp) */
int alpgpu_malloc(alpgpu_ctx* ctx, void** d_ptr, size_t bytes);
int alpgpu_free(alpgpu_ctx* ctx, void* d_ptr);
int alpgpu_memcpy_h2d(alpgpu_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int alpgpu_memcpy_d2h(alpgpu_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
int alpgpu_memset(alpgpu_ctx* ctx, void* d_dst, int value, size_t bytes);
/* page-locked host memory (copies to and from it are plain DMA) and a host-to-device copy that is enqueued but not waited for:
 * h_src must stay untouched until a later synchronous call on this context (alpgpu_memcpy_d2h, alpgpu_synchronize) has returned.
 * include/alp/batch.hpp moves a whole rowgroup's arrays with one copy each way through such a buffer. */
int alpgpu_malloc_host(alpgpu_ctx* ctx, void** h_ptr, size_t bytes);
int alpgpu_free_host(alpgpu_ctx* ctx, void* h_ptr);
int alpgpu_memcpy_h2d_async(alpgpu_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);

/* worst-case stream capacities for n_vectors (bytes) */
uint64_t alpgpu_packed_capacity(uint64_t n_vectors);
uint64_t alpgpu_exc_capacity(uint64_t n_vectors);

/* ---- whole-column hot path ----------------------------------------------------------------------- */

/* Rowgroup init for every rowgroup of the column: first-level sampling, (e,f) top-k search, scheme
 * decision, and for ALP_RD rowgroups the cut/dictionary search.  Writes col->d_rowgroups[0..n_rowgroups). */
int alpgpu_rowgroup_init_f64(alpgpu_ctx* ctx, const double* d_in, uint64_t n_vectors, alpgpu_column* col);

/* The same decision for ONE rowgroup from first-level samples the caller gathered (what the reference's
 * find_top_k_combinations, include/alp/encoder.hpp:139-235, and find_best_dictionary, include/alp/rd.hpp:89-104,
 * receive): d_samples holds n_samples (1..288) doubles, blocks of min(n_samples, 32) per sampled vector. */
int alpgpu_state_from_samples_f64(alpgpu_ctx* ctx, const double* d_samples, uint32_t n_samples, alpgpu_rowgroup_state* d_state);
/* rd_encoder::init's half alone (include/alp/rd.hpp:180-185): cut + dictionary for these samples, no ALP/ALP_RD re-decision */
int alpgpu_rd_state_from_samples_f64(alpgpu_ctx* ctx, const double* d_samples, uint32_t n_samples, alpgpu_rowgroup_state* d_state);
/* rd_encoder::build_left_parts_dictionary for ONE cut position (include/alp/rd.hpp:33-87, called by find_best_dictionary :89-104 for every cut
 * and once more for the chosen one): right_bit_width = 64 - cut for doubles (48..63), 32 - cut for floats (16..31).  *d_state receives the ALP_RD
 * state of that cut (bit widths, dictionary size, dictionary in the reference's order), *d_estimate the value the reference returns —
 * estimate_compression_size (rd.hpp:23-31): right + left bit width + 32 bits per sampled exception / sample.  Both in device memory. */
int alpgpu_rd_dictionary_for_cut_f64(alpgpu_ctx* ctx, const double* d_samples, uint32_t n_samples, uint8_t right_bit_width, alpgpu_rowgroup_state* d_state,
                                     double* d_estimate);
int alpgpu_rd_dictionary_for_cut_f32(alpgpu_ctx* ctx, const float* d_samples, uint32_t n_samples, uint8_t right_bit_width, alpgpu_rowgroup_state* d_state,
                                     double* d_estimate);

/* Vector encode of the whole column given col->d_rowgroups (from alpgpu_rowgroup_init_f64 or supplied by
 * the caller): second-level sampling, encode + exception compaction, analyze_ffor, FFOR pack (ALP);
 * split + dictionary encode + FFOR pack of right/left (ALP_RD).  Single pass over the input; output
 * offsets are assigned in vector order.  Writes d_vectors, d_packed, d_exc, d_totals.  If a stream is too small the
 * overflow flag is raised, nothing is written past the buffers and the column content is unspecified — but every vector
 * that did not fit gets an empty descriptor, so decoding such a column stays inside the buffers. */
int alpgpu_encode_vectors_f64(alpgpu_ctx* ctx, const double* d_in, uint64_t n_vectors, alpgpu_column* col);

/* alpgpu_rowgroup_init_f64 followed by alpgpu_encode_vectors_f64 */
int alpgpu_encode_f64(alpgpu_ctx* ctx, const double* d_in, uint64_t n_vectors, alpgpu_column* col);

/* Fused decode of the whole column: ALP vectors = falp (unFFOR + int->double) + patch_exceptions;
 * ALP_RD vectors = unFFOR(right,left) + dictionary glue + patch.  d_out receives n_vectors*1024 doubles.
 * TRUST: alpgpu_decode_* / alpgpu_decode_sum_* / alpgpu_decode_count_range_* / alpgpu_column_sum_* follow col->d_vectors as they
 * find it — offsets, widths and exception counts are NOT checked by the kernels (a descriptor with a bad packed_off reads out of
 * bounds).  Columns written by alpgpu_encode_* and columns loaded by alpgpu_column_from_blob / alpgpu_decompress_host_* (which
 * validate every descriptor on the host) are safe; for descriptors from anywhere else call alpgpu_column_validate first. */
int alpgpu_decode_f64(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_out);

/* Decode fused into a consumer (the SCAN/SUM shape of the reference's end-to-end bench,
 * publication/source_code/bench_end_to_end/src/benchmarks/alp/queries/q1.cpp:63-104): d_sums[v] = sum of the 1024 decoded
 * values of vector v, exceptions patched in; the doubles themselves never reach HBM.  Summation order (so that the result can
 * be reproduced bit for bit): wavefront q of 4 owns values 256q..256q+255; lane L of it adds its values 256q+2L, +1, 256q+128+2L,
 * +1 in that order starting from +0.0, giving p[q][L]; then s[L] = (p[0][L] + p[1][L]) + (p[2][L] + p[3][L]) for L = 0..63; then the
 * 64 s[L] combine by a balanced binary tree over ADJACENT lanes — (0,1), (2,3), ...; then (0..1, 2..3), ...; six levels.
 * (Earlier in round 3 each wavefront ran that tree over its own 64 partials first and the four results were combined last; round 2
 * used a butterfly.  The order is a property of the library version: tests/test_decode_sum_gpu.py holds the host replica.) */
int alpgpu_decode_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_sums);
/* The other consumer named there, a predicate pushed into the scan: d_counts[v] = number of decoded values x of vector v with
 * lo <= x <= hi (exceptions patched in; NaN never qualifies; -0.0 == 0.0 as in C).  Nothing but 4 bytes per vector is written. */
int alpgpu_decode_count_range_f64(alpgpu_ctx* ctx, const alpgpu_column* col, double lo, double hi, uint32_t* d_counts);

/* The column's total (the reference's consumer adds every vector into ONE accumulator, q1.cpp:91-100): *d_total (device memory,
 * one double) = the per-vector sums of alpgpu_decode_sum_* combined by a balanced binary tree over adjacent elements, absent
 * elements counting as +0.0: level by level, s'[i] = s[2i] + s[2i+1] over the array padded with +0.0 to a multiple of 1024, ten
 * levels per kernel launch, until one element is left.  (A chain of a million dependent adds has no parallel form with the same
 * rounding; this order is the documented replacement, reproduced on the host by tests/test_decode_sum_gpu.py.)  0.0 for an
 * empty column.  alpgpu_tree_sum_f64 is that tree over any device array of n doubles.  Asynchronous on the context's stream. */
int alpgpu_column_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_total);
int alpgpu_column_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_total);
int alpgpu_tree_sum_f64(alpgpu_ctx* ctx, const double* d_in, uint64_t n, double* d_total);

/* ---- random access ----------------------------------------------------------------------------------------------------
 * Value index r of a column = value r & 1023 of vector r >> 10 (ALPGPU_VECTOR_SIZE values per vector; tail padding included), so a column has
 * n_vectors * 1024 value indices.  (The names say "index" and "slice": a "row" is a FastLanes row inside a lane)  Each value
 * is read where it lies — its vector's descriptor, one or two packed words, for ALP_RD a left index and a dictionary entry, and a binary search
 * of the vector's exception positions — and no vector is decoded whole.
 *   alpgpu_gather_*        d_out[k] (k < n) = value d_idx[k]: bit for bit what alpgpu_decode_* writes at d_out[d_idx[k]], exceptions patched in
 *                          (NaN payloads, +-inf and -0.0 included).  Indices may come in any order and may repeat.  An index below 0 or at or above
 *                          n_vectors * 1024 gets the canonical quiet NaN, bits 0x7FF8000000000000 (float: 0x7FC00000), stored as an integer; nothing
 *                          is read for it.  d_idx: n int64 in device memory.
 *   alpgpu_decode_slice_*  d_out[k] (k < n) = value first + k, for any first — inside a vector or inside a rowgroup as well.  first + n greater than
 *                          n_vectors * 1024 (also when n == 0), or a first + n that overflows, returns ALPGPU_ERR_INVALID and nothing is enqueued (first
 *                          and n are host values: the check is made on the host).
 * Both: n == 0 with otherwise valid arguments returns ALPGPU_OK and launches nothing.  A NULL ctx, col or d_out with n > 0 (gather: or a NULL d_idx)
 * returns ALPGPU_ERR_INVALID.  One kernel launch, asynchronous on the context's stream; d_out needs no alignment beyond its value type.
 * TRUST: as for alpgpu_decode_f64, the descriptors are followed as found.  One more precondition: within each vector the exception positions
 * strictly ascend.  Every encoder of this library writes them so (as does the reference), and the store decode's rank lookup assumes it too, but
 * alpgpu_column_validate does not check the order.
 * Read-only and stateless: no host synchronisation, and none of what the context remembers about columns (segment tables, the learned sizes of
 * unhinted decodes, the progress word, the read-ahead) is read or written.  So both are safe inside a stream capture, and a decode planned before a
 * gather is planned the same way after it. */
int alpgpu_gather_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const int64_t* d_idx, uint64_t n, double* d_out);
int alpgpu_gather_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const int64_t* d_idx, uint64_t n, float* d_out);
int alpgpu_decode_slice_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, double* d_out);
int alpgpu_decode_slice_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, float* d_out);

/* ---- selection --------------------------------------------------------------------------------------------------------
 * A range predicate evaluated on the compressed column: which values qualify, as a list of value indices (the numbering of the random-access
 * section) that alpgpu_gather_* takes as it is — "filter on column A, fetch the matching values of column B" runs on compressed columns:
 * select_range(A) -> d_idx, gather(B, d_idx).  The decoded column never reaches device memory.
 * Predicate: value index r qualifies when first <= r < first + n and lo <= x <= hi for x = the decoded value, exceptions patched in — the
 *   comparison of alpgpu_decode_count_range_*: NaN never qualifies (as a value or as a bound), -0.0 == 0.0, lo > hi selects nothing, +-inf are
 *   ordinary bounds and ordinary values.  So over the whole column (first = 0, n = n_vectors * 1024) the number of selected indices of vector v
 *   is d_counts[v] of alpgpu_decode_count_range_* with the same bounds.
 * Output: *d_count (one uint64_t in device memory) = the number of qualifying values, also when it exceeds capacity.  d_idx[j] for
 *   j < min(*d_count, capacity) = the j-th qualifying index in ASCENDING order.  d_vals (may be NULL): d_vals[j] = that value, bit for bit what
 *   alpgpu_decode_* writes at d_out[d_idx[j]] (a selected -0.0 keeps its sign, a selected exception its bits).  Nothing is written at or behind
 *   capacity, and nothing at j >= *d_count.  The result is a function of the column and the arguments only: it does not depend on the launch
 *   shape, on how workgroups are scheduled or on the order they arrive in (positions come from a prefix sum, never from an atomic).
 * Range: first and n are host values and checked on the host like alpgpu_decode_slice_*: first + n greater than n_vectors * 1024, or
 *   overflowing, returns ALPGPU_ERR_INVALID and nothing is enqueued.  The tail padding of the last vector is excluded by passing n = n_values.
 *   n == 0 is valid: *d_count becomes 0 (that one write is enqueued).
 * Arguments: capacity == 0 is valid and makes the call a count (d_idx and d_vals may then be NULL).  A NULL ctx, col or d_count, a NULL
 *   d_scratch with n > 0, or a NULL d_idx with capacity > 0 returns ALPGPU_ERR_INVALID.
 * Scratch: caller-owned like every buffer of this ABI (the context's scan workspace grows by allocation and orders itself with events, which
 *   would make the call stateful).  alpgpu_select_scratch_bytes(col->n_vectors) bytes of device memory, 16-byte aligned; what they hold before
 *   does not matter, what they hold after is unspecified.  That is 12 bytes per vector (a u64 offset and a u32 count) plus the block sums of
 *   the prefix sum, in all at most 12 * n_vectors + n_vectors / 100 + 256 bytes (n_vectors above 2^54: UINT64_MAX); never 0.
 * Asynchronous and stateless, as the random access is: everything is enqueued on the context's stream and on that stream only (a captured graph
 *   gets no parallel branches), there is no host synchronisation and no allocation, and none of what the context remembers about columns
 *   (segment tables, the learned sizes of unhinted decodes, the progress word, the read-ahead) is read or written.  Safe inside a stream
 *   capture.  No workgroup waits for another: the phases (count per vector, prefix sum, emit) are separate launches.
 * Cost: the compressed column is read once, and once more for the vectors that hold a qualifying value; 8 (+ 8 or 4) bytes are written per
 *   selected value.
 * TRUST: as for alpgpu_decode_* and alpgpu_gather_* (descriptors followed as found; exception positions ascend within a vector). */
uint64_t alpgpu_select_scratch_bytes(uint64_t n_vectors);
int alpgpu_select_range_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, double lo, double hi, int64_t* d_idx, double* d_vals,
                            uint64_t capacity, uint64_t* d_count, void* d_scratch);
int alpgpu_select_range_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, float lo, float hi, int64_t* d_idx, float* d_vals,
                            uint64_t capacity, uint64_t* d_count, void* d_scratch);
/* debug / test: the selection's prefix sum alone, so that its deeper levels can be exercised without a column of millions of vectors.
 * d_offsets[i] = d_counts[0] + ... + d_counts[i - 1] (i < n, n > 0), *d_total = the sum of all n; d_scratch: alpgpu_select_scratch_bytes(n) bytes. */
int alpgpu_debug_select_scan(alpgpu_ctx* ctx, const uint32_t* d_counts, uint64_t n, uint64_t* d_offsets, uint64_t* d_total, void* d_scratch);

/* ---- zone maps --------------------------------------------------------------------------------------------------------
 * A zone map is one record {min, max} per vector of a column: a plain array in device memory, caller-allocated like every buffer of this ABI
 * and indexed by vector (alpgpu_zone_f64: 16 bytes, the array 16-byte aligned; alpgpu_zone_f32: 8 bytes, 8-byte aligned; a misaligned array,
 * or a d_in that is not 16-byte aligned, returns ALPGPU_ERR_INVALID).  It is not part of alpgpu_column
 * and not part of the serialized container: a caller who persists a blob keeps the n_vectors records beside it.
 * The record of vector v, defined bit for bit:
 *   - min / max range over the 1024 decoded values of the vector, exceptions patched in: exactly the values alpgpu_decode_* writes (the tail
 *     padding of the last vector included; it repeats a value of the vector, so it changes nothing);
 *   - NaNs are ignored, quiet and signalling alike, whatever their payload, in an exception record (ALP) as in the packed words (ALP_RD);
 *   - +-inf are ordinary values;
 *   - zeros are ordered -0.0 < +0.0 (IEEE 754-2019 minimumNumber / maximumNumber): a vector holding both zeros and nothing smaller has
 *     min = -0.0, sign bit set; the mirror image for max;
 *   - a vector without a single value that is not a NaN has the empty interval min = +inf, max = -inf.
 *   alpgpu_zone_map_*            the records of an encoded column: a third fused consumer beside alpgpu_decode_sum_* and
 *                                alpgpu_decode_count_range_* — each vector is decoded in registers by one wavefront and reduced to its two values;
 *                                nothing but the records is written.  d_zones: col->n_vectors records.
 *   alpgpu_zone_map_of_values_*  the same records from the raw values (d_in: n_vectors * 1024 values in device memory, 16-byte aligned), for a
 *                                caller who still holds them at encode time: one streaming read.  The codec is lossless, so this gives the same
 *                                bytes as alpgpu_zone_map_* of the encoded column.
 *   alpgpu_zones_minmax_*        the column's MIN / MAX: d_minmax[0] / d_minmax[1] (device memory) = the reduction of n_vectors records under the
 *                                same ordering; {+inf, -inf} for an empty column (n_vectors == 0: that write is still enqueued) or one of NaNs only.
 *                                Minimum and maximum are exactly associative and commutative, so the result is a function of the records alone
 *                                although workgroups join it with atomics; no scratch.
 *   alpgpu_select_range_zoned_*  alpgpu_select_range_* with the zone map of the column (col->n_vectors records, whatever first and n are).  Contract,
 *                                scratch (alpgpu_select_scratch_bytes), argument checks, ordering, determinism and capture-safety are those of
 *                                alpgpu_select_range_*; in addition a NULL d_zones with n > 0 returns ALPGPU_ERR_INVALID.  The count pass reads a
 *                                vector's record first:
 *                                  excluded   !(max >= lo && min <= hi) (a NaN bound excludes everything): the vector counts 0; its descriptor,
 *                                             packed words and exception record are not read;
 *                                  contained  min >= lo && max <= hi and the vector cannot hold a NaN (an ALP vector without exceptions; ALP_RD
 *                                             vectors never take this arm): the vector counts its whole share of [first, first + n) after its
 *                                             descriptor alone, and the emit pass writes its indices without decoding when no values are wanted;
 *                                  otherwise  the vector is decoded as in alpgpu_select_range_*.
 *                                GUARANTEE: for any zone map in which every vector's record contains that vector's true interval, the call
 *                                returns bit for bit what alpgpu_select_range_* returns — exact records, widened records and {-inf, +inf}
 *                                everywhere alike.  A record that is too narrow gives a wrong selection but never an out-of-bounds access: a
 *                                record only ever makes the kernel read less.
 * All of them: everything is enqueued on the context's stream and on that stream only, asynchronous, no host synchronisation, no allocation, and
 *   none of what the context remembers about columns is read or written; safe inside a stream capture.  n_vectors == 0 (for alpgpu_zone_map_*:
 *   col->n_vectors == 0) is ALPGPU_OK and, except for the reset of alpgpu_zones_minmax_*, launches nothing.  A NULL ctx, col, d_in, d_zones or
 *   d_minmax with n_vectors > 0 returns ALPGPU_ERR_INVALID.
 * TRUST: alpgpu_zone_map_* and alpgpu_select_range_zoned_* as for alpgpu_decode_* (descriptors followed as found). */
typedef struct alpgpu_zone_f64 {
	double min, max;
} alpgpu_zone_f64;
typedef struct alpgpu_zone_f32 {
	float min, max;
} alpgpu_zone_f32;
int alpgpu_zone_map_f64(alpgpu_ctx* ctx, const alpgpu_column* col, alpgpu_zone_f64* d_zones);
int alpgpu_zone_map_f32(alpgpu_ctx* ctx, const alpgpu_column* col, alpgpu_zone_f32* d_zones);
int alpgpu_zone_map_of_values_f64(alpgpu_ctx* ctx, const double* d_in, uint64_t n_vectors, alpgpu_zone_f64* d_zones);
int alpgpu_zone_map_of_values_f32(alpgpu_ctx* ctx, const float* d_in, uint64_t n_vectors, alpgpu_zone_f32* d_zones);
int alpgpu_zones_minmax_f64(alpgpu_ctx* ctx, const alpgpu_zone_f64* d_zones, uint64_t n_vectors, double* d_minmax);
int alpgpu_zones_minmax_f32(alpgpu_ctx* ctx, const alpgpu_zone_f32* d_zones, uint64_t n_vectors, float* d_minmax);
int alpgpu_select_range_zoned_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const alpgpu_zone_f64* d_zones, uint64_t first, uint64_t n, double lo, double hi,
                                  int64_t* d_idx, double* d_vals, uint64_t capacity, uint64_t* d_count, void* d_scratch);
int alpgpu_select_range_zoned_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const alpgpu_zone_f32* d_zones, uint64_t first, uint64_t n, float lo, float hi,
                                  int64_t* d_idx, float* d_vals, uint64_t capacity, uint64_t* d_count, void* d_scratch);

/* ---- selection bitmaps -------------------------------------------------------------------------------------------------
 * The qualify mask of a range predicate, kept instead of counted away: predicates on several columns of equal length combine in it (AND, OR), and
 * only what is left at the end is listed (alpgpu_mask_to_indices), projected (alpgpu_decode_masked_*) or summed (alpgpu_decode_sum_masked_*):
 *   WHERE lo1 <= a <= hi1 AND lo2 <= b <= hi2   select_mask(a, SET), select_mask(b, AND);   SUM(c) WHERE ...: decode_sum_masked(c), tree_sum;
 *   SELECT c, d WHERE ...: decode_masked(c), decode_masked(d).
 * The bitmap of a column is n_vectors * 16 uint64_t words in device memory, caller-owned like every buffer of this ABI and 8-byte aligned (a
 *   misaligned pointer returns ALPGPU_ERR_INVALID): bit r & 63 of word r >> 6 stands for value index r, the numbering of the random-access section,
 *   so vector v owns words 16 v .. 16 v + 15 (128 bytes).  It is not part of alpgpu_column and not part of the serialized container.
 *   alpgpu_select_mask_*        Let q(r) = first <= r < first + n and lo <= x_r <= hi: exactly the predicate of alpgpu_select_range_* (NaN never
 *                               qualifies, as a value or as a bound; -0.0 == 0.0; lo > hi selects nothing; +-inf are ordinary values and bounds;
 *                               exceptions patched in, the store decode's arithmetic).  For EVERY value index r of the column:
 *                                 op = ALPGPU_MASK_SET  bit(r) = q(r): every word of the bitmap is written, what it held does not matter;
 *                                 op = ALPGPU_MASK_AND  bit(r) &= q(r): bits outside [first, first + n) clear;
 *                                 op = ALPGPU_MASK_OR   bit(r) |= q(r): bits outside the range keep their value;
 *                               any other op returns ALPGPU_ERR_INVALID and enqueues nothing.  Cost: one launch, one wavefront per vector.  A vector
 *                               outside the range is settled from its 128 bytes of bitmap; under AND a vector whose 16 words are all zero, and
 *                               under OR one whose 16 words are all ones, is not decoded — its descriptor, packed words and exception record are
 *                               not read — so a second predicate costs in proportion to what the first left open.
 *                               Range: checked on the host as in alpgpu_select_range_* (first + n past n_vectors * 1024, or overflowing:
 *                               ALPGPU_ERR_INVALID, nothing enqueued).  n == 0 is valid: SET and AND clear the bitmap, OR enqueues nothing.
 *                               col->n_vectors == 0 is ALPGPU_OK and launches nothing.  A NULL ctx or col, or a NULL d_mask with n_vectors > 0,
 *                               returns ALPGPU_ERR_INVALID.
 *   alpgpu_mask_to_indices      the set bits of a bitmap of n_vectors vectors as ASCENDING value indices: *d_count = their number, also when it
 *                               exceeds capacity; d_idx[j] for j < min(*d_count, capacity) = the j-th; nothing is written at or behind capacity.
 *                               capacity == 0 makes it a count (d_idx may be NULL).  d_scratch: alpgpu_select_scratch_bytes(n_vectors) bytes,
 *                               16-byte aligned, as for the selection.  Three launches ordered by kernel boundaries (per-vector popcount, the
 *                               selection's prefix sum, emit); positions come from the prefix sum and v_mbcnt ranks, never from an atomic.
 *                               n_vectors == 0 writes *d_count = 0.  For a bitmap made by alpgpu_select_mask_* with op = SET the result is bit
 *                               for bit that of alpgpu_select_range_* with the same arguments.
 *   alpgpu_decode_sum_masked_*  d_sums[v] = the sum of the decoded values of vector v whose bit is set, d_counts[v] (may be NULL) = the number of
 *                               set bits of the vector (AVG needs nothing else); the values never reach HBM.  A vector whose 16 words are zero
 *                               gets +0.0 and 0 and is not read.  Summation order (so that the result can be reproduced bit for bit): lane L of
 *                               64 starts from +0.0 and, for m = 0..15 in that order, adds value 64 m + L if its bit is set and does nothing
 *                               otherwise (float values widen to double first, exactly); the 64 partials combine by the balanced binary tree over
 *                               adjacent lanes of alpgpu_decode_sum_* — (0,1), (2,3), ...; six levels.  No multiplication is involved, nothing can
 *                               contract.  This order belongs to THIS entry point; it is not that of alpgpu_decode_sum_*: a full bitmap gives the
 *                               same mathematical sum, not necessarily the same bits.  The column's total is alpgpu_tree_sum_f64 over d_sums.  A
 *                               selected NaN makes its vector's sum a NaN of unspecified payload (bitmaps made by alpgpu_select_mask_* never select
 *                               one; a caller-made bitmap may).  (tests/test_mask_gpu.py holds the host replica.)
 *  -- masked projection --
 *   alpgpu_decode_masked_*      the column's values at the set bits of a bitmap, compacted in ascending index order: the projection of
 *                               SELECT c WHERE ..., one in-register decode of each vector that holds a set bit instead of alpgpu_mask_to_indices and
 *                               a gather.  d_mask: col->n_vectors * 16 words; every bit is honoured as found, over all n_vectors * 1024 indices
 *                               (a bitmap built with n = n_values has the tail padding clear); it is read and never written.  Output as
 *                               alpgpu_select_range_* with d_vals: *d_count = the number of set bits, also when it exceeds capacity; for
 *                               j < min(*d_count, capacity), d_vals[j] = the value at the j-th set bit, bit for bit what alpgpu_decode_* writes at that
 *                               index (an exception keeps its bits, -0.0 its sign, a NaN its payload), and d_idx[j] (d_idx may be NULL) = that
 *                               index, as alpgpu_mask_to_indices returns it.  Nothing is written at or behind capacity, nothing at j >= *d_count.
 *                               capacity == 0 makes the call a count (d_vals and d_idx may be NULL).  d_scratch: alpgpu_select_scratch_bytes(
 *                               col->n_vectors) bytes, 16-byte aligned, the selection's layout, contents unspecified afterwards.  Three phases
 *                               ordered by kernel boundaries: per-vector popcount, the selection's prefix sum, emit (one wavefront per vector);
 *                               positions come from the prefix sum, the popcount of the words before and v_mbcnt, never from an atomic.  Cost of
 *                               the emit pass: a vector without a set bit 4 bytes, one at or behind the capacity 12; any other its 128 bytes of
 *                               bitmap, its descriptor and exception positions, and the packed words and exception values of each half (8 words
 *                               of bitmap, 512 values) that holds a set bit; it stops behind the vector's last set bit.
 *                               A NULL ctx, col, d_mask or d_count, a d_mask that is not 8-byte aligned, a NULL d_scratch with n_vectors > 0 and a
 *                               NULL d_vals with capacity > 0 return ALPGPU_ERR_INVALID before anything is enqueued.  col->n_vectors == 0 writes
 *                               *d_count = 0 and returns ALPGPU_OK.
 * All of them: everything is enqueued on the context's stream and on that stream only, asynchronous, no host synchronisation, no allocation, none
 *   of what the context remembers about columns is read or written; safe inside a stream capture.  The result is a function of the column, the
 *   bitmap and the arguments alone.
 * TRUST: as for alpgpu_select_range_* (descriptors followed as found; exception positions ascend within a vector). */
#define ALPGPU_MASK_SET 0
#define ALPGPU_MASK_AND 1
#define ALPGPU_MASK_OR 2
int alpgpu_select_mask_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, double lo, double hi, int op, uint64_t* d_mask);
int alpgpu_select_mask_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, float lo, float hi, int op, uint64_t* d_mask);
int alpgpu_mask_to_indices(alpgpu_ctx* ctx, const uint64_t* d_mask, uint64_t n_vectors, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch);
int alpgpu_decode_sum_masked_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts);
int alpgpu_decode_sum_masked_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts);
int alpgpu_decode_masked_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, double* d_vals, int64_t* d_idx, uint64_t capacity, uint64_t* d_count,
                             void* d_scratch);
int alpgpu_decode_masked_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, float* d_vals, int64_t* d_idx, uint64_t capacity, uint64_t* d_count,
                             void* d_scratch);

/* ---- two-column consumers ----------------------------------------------------------------------------------------------
 * Two columns a and b of equal length (a->n_vectors == b->n_vectors; both of the entry point's type, mixed f64 / f32 pairs are not offered),
 * decoded side by side: one wavefront decodes vector v of a AND vector v of b in registers and combines them lane by lane, so that neither
 * column's values reach HBM.  A predicate between columns, and the aggregate of a product under a bitmap (TPC-H Q6):
 *   WHERE a < b                         compare_mask(a, b, LT, SET);   WHERE lo <= c <= hi AND a >= b: select_mask(c, SET), compare_mask(a, b, GE, AND);
 *   SUM(a * b) WHERE ...                select_mask ... ; decode_dot_masked(a, b); tree_sum.
 * The bitmap is that of the section above (n_vectors * 16 words, 8-byte aligned, bit r & 63 of word r >> 6 = value index r).  a_r and b_r are
 * the values alpgpu_decode_* writes at index r, exceptions patched in.  a == b (the same column) is allowed.
 *   alpgpu_compare_mask_*       Let q(r) = first <= r < first + n and a_r CMP b_r, CMP one of ALPGPU_CMP_LT / _LE / _GT / _GE / _EQ / _NE with the
 *                               meaning of C's <, <=, >, >=, ==, !=: a NaN on either side makes LT, LE, GT, GE and EQ false and NE true;
 *                               -0.0 == 0.0; +-inf are ordinary values.  op = ALPGPU_MASK_SET / _AND / _OR with exactly the meaning, the range
 *                               check and the skip rules of alpgpu_select_mask_*: SET writes every word of the bitmap, AND clears the bits
 *                               outside the range, OR leaves them; a vector outside the range is settled from its 128 bytes of bitmap; under
 *                               AND a vector whose 16 words are all zero, and under OR one whose 16 words are all ones, is settled the same
 *                               way — neither column's descriptor, packed words or exception record is read.  n == 0: SET and AND clear the
 *                               bitmap, OR enqueues nothing.  first + n past n_vectors * 1024, or overflowing: ALPGPU_ERR_INVALID, nothing enqueued.
 *                               An unknown cmp or op returns ALPGPU_ERR_INVALID and enqueues nothing.
 *   alpgpu_decode_dot_masked_*  d_sums[v] = the sum, over the set bits of vector v, of a_r * b_r; d_counts[v] (may be NULL) = the number of set
 *                               bits.  A vector whose 16 words are zero gets +0.0 and 0, and neither column is read for it.  Summation order (so
 *                               that the result can be reproduced bit for bit): lane L of 64 starts from +0.0 and, for m = 0..15 in that order,
 *                               if bit 64 m + L is set, forms t = a * b rounded once to double (float values widen to double first, exactly;
 *                               their product is then exact) and acc = acc + t rounded once — two operations, never a fused multiply-add —
 *                               and does nothing if the bit is clear; the 64 partials combine by the balanced binary tree over adjacent lanes
 *                               of alpgpu_decode_sum_* — (0,1), (2,3), ...; six levels.  The column's total is alpgpu_tree_sum_f64 over d_sums.  A
 *                               selected NaN, or inf * 0, makes its vector's sum a NaN of unspecified payload.  d_mask is read and never
 *                               written; d_mask and d_sums are required.  (tests/pair_replica.py holds the host replica.)
 * Both: a->n_vectors != b->n_vectors, a NULL ctx, a or b, a NULL d_mask (or d_sums) with n_vectors > 0 and a d_mask that is not 8-byte aligned
 *   return ALPGPU_ERR_INVALID before anything is enqueued; n_vectors == 0 is ALPGPU_OK and launches nothing.  One launch, one wavefront per
 *   vector pair, on the context's stream and on that stream only; asynchronous, no host synchronisation, no allocation, no atomics on results,
 *   none of what the context remembers about columns is read or written; safe inside a stream capture.  The result is a function of the two
 *   columns, the bitmap and the arguments alone.
 * TRUST: as for alpgpu_select_range_* (descriptors followed as found; exception positions ascend within a vector), for both columns. */
#define ALPGPU_CMP_LT 0
#define ALPGPU_CMP_LE 1
#define ALPGPU_CMP_GT 2
#define ALPGPU_CMP_GE 3
#define ALPGPU_CMP_EQ 4
#define ALPGPU_CMP_NE 5
int alpgpu_compare_mask_f64(alpgpu_ctx* ctx, const alpgpu_column* a, const alpgpu_column* b, uint64_t first, uint64_t n, int cmp, int op, uint64_t* d_mask);
int alpgpu_compare_mask_f32(alpgpu_ctx* ctx, const alpgpu_column* a, const alpgpu_column* b, uint64_t first, uint64_t n, int cmp, int op, uint64_t* d_mask);
int alpgpu_decode_dot_masked_f64(alpgpu_ctx* ctx, const alpgpu_column* a, const alpgpu_column* b, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts);
int alpgpu_decode_dot_masked_f32(alpgpu_ctx* ctx, const alpgpu_column* a, const alpgpu_column* b, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts);

/* ---- grouped aggregation -----------------------------------------------------------------------------------------------------------------
 * SELECT key, SUM(x), COUNT(*) ... WHERE ... GROUP BY key (TPC-H Q1), and the histogram of a column under a predicate: per-group SUM and COUNT
 * of a value column by closed ranges of a key column, in ONE pass that decodes vector v of both columns in the registers of one wavefront and
 * settles every group there.  G groups cost two decodes, not the 2 G of G rounds of bitmap copy + select_mask(AND) + decode_sum_masked.
 *   WHERE ...                           select_mask / compare_mask ... into the bitmap (all ones for no WHERE clause);
 *   SUM(x), COUNT(*) GROUP BY key       decode_group_sum(val, key, bitmap, lo, hi); group_totals.
 *   alpgpu_decode_group_sum_*   val and key: two columns of the entry point's type with equal n_vectors; val == key is allowed (a histogram
 *                               with per-bin sums).  d_mask: the selection bitmap of the sections above (n_vectors * 16 words, 8-byte aligned),
 *                               required, read and never written.  lo, hi: HOST arrays of n_groups bounds, 1 <= n_groups <= ALPGPU_GROUP_MAX;
 *                               group g is the closed range lo[g] <= k <= hi[g] with exactly the predicate of alpgpu_select_mask_*: a NaN never
 *                               qualifies, as a value or as a bound; -0.0 == 0.0; lo > hi selects nothing; +-inf are ordinary.  The arrays are
 *                               read before the call returns and travel as kernel arguments (at most 256 bytes), so a captured graph keeps the
 *                               bounds it was captured with.  Groups are independent: they may overlap (a value then counts in each group it
 *                               falls in), touch or be empty; a discrete key is lo[g] == hi[g]; adjacent histogram bins are the caller's business.
 *                               Output, group-major: d_sums[g * n_vectors + v] and d_counts[g * n_vectors + v] (d_counts may be NULL); every (g, v)
 *                               with g < n_groups is written and nothing else.
 *                               The contract, bit for bit: let M_g be the caller's bitmap ANDed with alpgpu_select_mask_*(key, first = 0,
 *                               n = n_vectors * 1024, lo[g], hi[g]); row g of d_sums and d_counts is what alpgpu_decode_sum_masked_*(val, M_g)
 *                               writes.  Summation order: lane L of 64 starts from +0.0; for m = 0..15 in that order it adds value 64 m + L of
 *                               val (a float widened to double first) if its bit is set and the key there is in range, and does nothing
 *                               otherwise; the 64 partials combine by the adjacent-lane tree of alpgpu_decode_sum_*.  No multiplication is
 *                               involved.  A selected NaN in val makes that sum a NaN of unspecified payload.  A vector whose 16 bitmap words
 *                               are zero gets +0.0 and 0 in every group, and neither column is read for it.  (tests/group_replica.py holds the
 *                               host replica.)
 *                               ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx, val, key, lo or hi; n_groups == 0 or
 *                               > ALPGPU_GROUP_MAX; unequal n_vectors; an implausible n_vectors; with n_vectors > 0 a NULL d_mask or d_sums, a
 *                               d_mask that is not 8-byte aligned, or columns without descriptors.  n_vectors == 0 is ALPGPU_OK and launches nothing.
 *   alpgpu_group_totals         d_sums, d_counts: [n_groups][n_vectors] as written above.  d_total_sums[g] is, bit for bit,
 *                               alpgpu_tree_sum_f64(d_sums + g * n_vectors, n_vectors); d_total_counts[g] is the exact integer sum of row g of
 *                               d_counts.  d_counts and d_total_counts are NULL together.  d_scratch is the caller's:
 *                               alpgpu_group_totals_scratch_bytes(n_vectors, n_groups) bytes, 16-byte aligned (it is used, and checked, only
 *                               when n_vectors > 1024); nothing is allocated and the context's workspace is not used.  No floating-point atomics.
 *                               n_vectors == 0 writes +0.0 and 0 and looks at neither input (their pointers may be NULL).  A NULL ctx or
 *                               d_total_sums, n_groups out of range and, with n_vectors > 0, a NULL d_sums and counts without their totals (or
 *                               the reverse) return ALPGPU_ERR_INVALID before anything is enqueued.
 * Both run on the context's stream and on that stream only: asynchronous, no host synchronisation, no allocation; none of what the context
 *   remembers about columns is read or written; safe inside a stream capture.  The result is a function of the arguments alone.
 * TRUST: as for alpgpu_select_range_* (descriptors followed as found; exception positions ascend within a vector), for both columns. */
#define ALPGPU_GROUP_MAX 16
int alpgpu_decode_group_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const double* lo, const double* hi,
                                uint32_t n_groups, double* d_sums, uint32_t* d_counts);
int alpgpu_decode_group_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const float* lo, const float* hi,
                                uint32_t n_groups, double* d_sums, uint32_t* d_counts);
size_t alpgpu_group_totals_scratch_bytes(uint64_t n_vectors, uint32_t n_groups);
int    alpgpu_group_totals(alpgpu_ctx* ctx, const double* d_sums, const uint32_t* d_counts, uint64_t n_vectors, uint32_t n_groups, double* d_total_sums,
                           uint64_t* d_total_counts, void* d_scratch);

/* ---- masked and grouped MIN / MAX --------------------------------------------------------------------------------------------------------
 * SELECT MIN(x), MAX(x) ... WHERE ..., and SELECT key, MIN(x), MAX(x), COUNT(*) ... WHERE ... GROUP BY key (TPC-H Q2, Q15): the two aggregates
 * the sections above leave out, computed like their sums — each vector decoded in the registers of one wavefront, no value reaching HBM.
 *   WHERE ...                           select_mask / compare_mask ... into the bitmap (all ones for no WHERE clause);
 *   MIN(x), MAX(x)                      decode_minmax_masked(x, bitmap); zones_minmax.
 *   MIN(x), MAX(x) GROUP BY key         decode_group_minmax(x, key, bitmap, lo, hi); group_minmax_totals.
 * The records are alpgpu_zone_f64 / alpgpu_zone_f32 of the zone-map section, with its alignment (16 / 8 bytes; a misaligned array returns
 * ALPGPU_ERR_INVALID) and its rules, bit for bit, over the SELECTED values: NaNs, quiet and signalling, are ignored; +-inf are ordinary values;
 * -0.0 < +0.0; {+inf, -inf} when no selected value is a number.  A float column gives float records: nothing widens.  Minimum and maximum are
 * exactly associative and commutative, so every result here is a function of the inputs alone and there is no order to document.
 * These records are NOT a zone map for alpgpu_select_range_zoned_*: they are narrower than the vector's true interval.
 *   alpgpu_decode_minmax_masked_*   d_zones[v] = {min, max} over the decoded values of vector v whose bit is set in d_mask (col->n_vectors * 16
 *                                   words, 8-byte aligned; every bit honoured as found; read and never written).  d_counts[v] (may be NULL) = the
 *                                   number of set bits of the vector, selected NaNs included, exactly as alpgpu_decode_sum_masked_* counts them.  A
 *                                   vector whose 16 words are zero gets {+inf, -inf} and 0, and the column is not read for it.  Under a full bitmap
 *                                   the records are bit for bit those of alpgpu_zone_map_*.  The column's MIN / MAX is alpgpu_zones_minmax_* over
 *                                   the records.
 *                                   ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx or col, a d_mask that is not 8-byte aligned,
 *                                   misaligned records and, with n_vectors > 0, a NULL d_mask or d_zones, an implausible n_vectors or a column
 *                                   without descriptors.  col->n_vectors == 0 is ALPGPU_OK and launches nothing.
 *   alpgpu_decode_group_minmax_*    The arguments of alpgpu_decode_group_sum_* with the same meaning: val and key of the entry point's type with
 *                                   equal n_vectors (val == key allowed); lo, hi HOST arrays of n_groups bounds, 1 <= n_groups <= ALPGPU_GROUP_MAX,
 *                                   read before the call returns and passed as kernel arguments; group g is lo[g] <= k <= hi[g] with the predicate
 *                                   of alpgpu_select_mask_* (a NaN never qualifies, as a key or as a bound; -0.0 == 0.0; lo > hi selects nothing);
 *                                   groups may overlap, touch or be empty.  Output, group-major: d_zones[g * n_vectors + v] and
 *                                   d_counts[g * n_vectors + v] (d_counts may be NULL); every (g, v) with g < n_groups is written and nothing else.
 *                                   The contract, bit for bit: let M_g be the caller's bitmap ANDed with alpgpu_select_mask_*(key, first = 0,
 *                                   n = n_vectors * 1024, lo[g], hi[g]); row g of d_zones is what alpgpu_decode_minmax_masked_*(val, M_g) writes, and
 *                                   row g of d_counts what alpgpu_decode_group_sum_* writes.  A vector whose 16 bitmap words are zero gets
 *                                   {+inf, -inf} and 0 in every row, and neither column is read for it.
 *                                   ALPGPU_ERR_INVALID before anything is enqueued: as alpgpu_decode_group_sum_*, and misaligned records.
 *                                   n_vectors == 0 is ALPGPU_OK and launches nothing.
 *   alpgpu_group_minmax_totals_*    d_zones: [n_groups][n_vectors] as written above.  d_minmax[2 g], d_minmax[2 g + 1] (device memory, 2 * n_groups
 *                                   values) are what alpgpu_zones_minmax_*(d_zones + g * n_vectors, n_vectors) writes: one call serves all groups.
 *                                   n_vectors == 0 writes {+inf, -inf} for every group (that write is still enqueued; d_zones may be NULL).  No
 *                                   scratch.  A NULL ctx or d_minmax, n_groups out of range, misaligned pointers and, with n_vectors > 0, a NULL
 *                                   d_zones return ALPGPU_ERR_INVALID before anything is enqueued.
 * All run on the context's stream and on that stream only: asynchronous, no host synchronisation, no allocation; none of what the context
 *   remembers about columns is read or written; safe inside a stream capture.  (tests/minmax_replica.py holds the host replica.)
 * TRUST: as for alpgpu_select_range_* (descriptors followed as found; exception positions ascend within a vector), for every column. */
int alpgpu_decode_minmax_masked_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, alpgpu_zone_f64* d_zones, uint32_t* d_counts);
int alpgpu_decode_minmax_masked_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, alpgpu_zone_f32* d_zones, uint32_t* d_counts);
int alpgpu_decode_group_minmax_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const double* lo, const double* hi,
                                   uint32_t n_groups, alpgpu_zone_f64* d_zones, uint32_t* d_counts);
int alpgpu_decode_group_minmax_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const float* lo, const float* hi,
                                   uint32_t n_groups, alpgpu_zone_f32* d_zones, uint32_t* d_counts);
int alpgpu_group_minmax_totals_f64(alpgpu_ctx* ctx, const alpgpu_zone_f64* d_zones, uint64_t n_vectors, uint32_t n_groups, double* d_minmax);
int alpgpu_group_minmax_totals_f32(alpgpu_ctx* ctx, const alpgpu_zone_f32* d_zones, uint64_t n_vectors, uint32_t n_groups, float* d_minmax);

/* ---- set membership -------------------------------------------------------------------------------------------------------------------------
 * `x IN (list)` on a compressed column into a selection bitmap: the predicate against a SET of values that the range and the two-column predicates
 * above cannot express (TPC-H Q12, Q16, Q19, Q22), and the probe side of a semi-join WHERE key IN (SELECT key FROM other WHERE ...), whose build
 * side is what alpgpu_decode_masked_* of the other column hands back, sorted:
 *   WHERE mode IN (3, 5)                        select_in_mask(mode, list, SET);   ... AND lo <= c <= hi: select_mask(c, AND);
 *   WHERE key IN (SELECT key FROM o WHERE ...)  select_mask(o.c ...); decode_masked(o.key, bitmap); sort; select_in_mask(key, list, AND or SET).
 * It belongs to the selection-bitmap family: the bitmap, op, first and n are those of alpgpu_select_mask_*.
 *   alpgpu_select_in_mask_*     member(x) is true iff some j < n_list has d_list[j] == x under C's ==: -0.0 and +0.0 match each other, a NaN (value
 *                               or list element) never matches, +-inf are ordinary.  q(r) = first <= r < first + n && (member(x_r) != (negate != 0)),
 *                               so under negate a NaN value inside the range qualifies: it is not a member.  x_r is, bit for bit, what
 *                               alpgpu_decode_* writes at r, exceptions patched in.  op, first and n have exactly the meaning, the host-side range
 *                               check and the n == 0 behaviour of alpgpu_select_mask_*, and the skip rules are the same: a vector outside the
 *                               range, one that is all-zero under AND and one that is all-ones under OR costs its 128 bytes of bitmap and nothing
 *                               of the column.  SET and AND cover every vector, OR only those of the range.
 *                               d_list: n_list elements of the column's type in DEVICE memory, aligned to the element, read when the kernel runs
 *                               (a captured graph sees the list's contents at replay; n_list and the pointers are fixed at capture).  It must be
 *                               sorted as numpy.sort sorts: ascending by <, -0.0 and +0.0 in either order, duplicates allowed, NaNs, if any, last.
 *                               A list that is not sorted gives unspecified bits and never a read outside d_list[0 .. n_list) nor a write outside
 *                               the bitmap: every probe index is clamped.  n_list == 0 is valid (d_list may be NULL): nothing is a member.
 *                               n_list > 2^31 - 1 returns ALPGPU_ERR_INVALID.
 *                               d_zones (may be NULL): the column's zone map, one record per vector (alpgpu_zone_map_*; 16 / 8 bytes aligned).  A
 *                               vector whose [min, max] holds no list element — the first element >= min is > max, or there is none — is settled
 *                               without reading its descriptor, packed words or exception record: as "nothing qualifies" without negate, as
 *                               "every index of its share of [first, first + n) qualifies" with it (NaNs included: they qualify anyway).  For a
 *                               vector that is decoded, the two searches that made the check give the part [j0, j1) of the list that can match,
 *                               and the per-value search runs over that part only.  The contract is that of alpgpu_select_range_zoned_*: any zone
 *                               map that contains the vectors' true intervals gives the bytes of the call without zones.  Records are read as
 *                               found; a NaN bound means "decode the vector".
 *                               Cost: one launch of persistent workgroups, sized to the device and not to the column.  A workgroup stages the
 *                               list into LDS once; a list of up to alpgpu_in_list_lds_max(value bytes) elements sits there whole and a value
 *                               costs ceil(log2(n_list + 1)) LDS probes and one ==; a longer one leaves every ceil(n_list / lds_max)-th element
 *                               there and the last ceil(log2(stride)) probes of each search read the list itself (L2-resident up to a few MiB).
 *                               ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx or col, a NULL d_mask (with n_vectors > 0) or one not
 *                               8-byte aligned, a NULL d_list with n_list > 0, a misaligned d_list or d_zones, an unknown op, a range past the
 *                               end.  col->n_vectors == 0 is ALPGPU_OK and launches nothing.
 *   alpgpu_in_list_lds_max      the longest list the kernel holds whole in LDS, for value_bytes 8 (4096) and 4 (8192); 0 for anything else.
 * The call runs on the context's stream and on that stream only: asynchronous, no host synchronisation, no allocation, no state kept, no atomics on
 *   results; none of what the context remembers about columns (the decode plans) is read or written; safe inside a stream capture.  The result is a
 *   function of the column, the list, the prior bitmap and the arguments alone.  (tests/in_list_replica.py holds the host replica.)
 * TRUST: as for alpgpu_select_range_* (descriptors followed as found; exception positions ascend within a vector). */
int    alpgpu_select_in_mask_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const double* d_list, uint64_t n_list, int negate,
                                 const alpgpu_zone_f64* d_zones, int op, uint64_t* d_mask);
int    alpgpu_select_in_mask_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const float* d_list, uint64_t n_list, int negate,
                                 const alpgpu_zone_f32* d_zones, int op, uint64_t* d_mask);
size_t alpgpu_in_list_lds_max(int value_bytes);

/* ---- top-k -----------------------------------------------------------------------------------------------------------------------------------
 * SELECT x ... WHERE ... ORDER BY x [DESC] LIMIT k (TPC-H Q2, Q3, Q10, Q18, Q21; "the 100 largest readings where ..."): the k largest or smallest
 * selected values of a compressed column and their indices, no value reaching HBM but the candidates of at most k vectors.
 *   WHERE ...                           select_mask / compare_mask / select_in_mask ... into the bitmap (all ones for no WHERE clause);
 *   ORDER BY x DESC LIMIT k             top_k(x, bitmap, k, largest = 1).
 * THE ORDER is the zone records' order made total:
 *   - NaNs are never returned, quiet or signalling, in an exception record as in packed words;
 *   - -inf < ... < -0.0 < +0.0 < ... < +inf: the two zeros are distinct and ordered;
 *   - equal bit patterns are ordered by ascending value index.
 *   As an integer: okey(x) = bits ^ (sign ? all-ones : sign-bit), an unsigned monotone bijection on the bits of the values that are not NaNs.  An
 *   element's composite key is (okey(x), ~index) for `largest` and (~okey(x), ~index) for smallest; no two elements of a column share one, so every
 *   step of the call is exact and free of ties, and the value's bits are recovered from the key.
 *   alpgpu_top_k_*              *d_count = min(k, number of set bits whose value is not a NaN).  For j < *d_count, d_vals[j] / d_idx[j] (d_idx may be
 *                               NULL) are the j-th element in descending composite order: with largest != 0 the largest value first, otherwise the
 *                               smallest first, equal bit patterns by ascending index.  d_vals[j] is bit for bit what alpgpu_decode_* writes at
 *                               d_idx[j]: a -0.0 keeps its sign, an exception its bits.  Nothing is written at j >= *d_count.  The result is a
 *                               function of the column, the bitmap, k and largest alone, not of launch shapes or of the order in which wavefronts
 *                               arrive.
 *                               d_mask: a selection bitmap of col->n_vectors * 16 words, 8-byte aligned, required, read and never written; the
 *                               caller excludes the tail padding by it, as with alpgpu_decode_masked_*.
 *                               d_records (may be NULL; 16-byte aligned): the EXACT masked records of this column under this bitmap — what
 *                               alpgpu_decode_minmax_masked_* writes, or, under a bitmap that selects every real value, what alpgpu_zone_map_*
 *                               writes.  With them the first decode pass is skipped; with NULL the call computes them into the scratch.  Records
 *                               that are not those give an UNSPECIFIED selection: unlike alpgpu_select_range_zoned_*, widened records are NOT
 *                               enough, because the vectors to decode are chosen by the k-th largest ATTAINED maximum (minimum).  Even then the
 *                               call writes at most k entries and reads and writes nothing out of bounds: the vectors it decodes are chosen by the
 *                               composite key (record, ~vector), so there are at most k of them whatever the records say.
 *                               Cost: without records one pass of alpgpu_decode_minmax_masked_*; then a histogram and a pick launch per byte of
 *                               the keys over the records (16 bytes per vector each), the decode of at most k vectors, the same over at most
 *                               min(k, n_vectors) * 1024 candidates, and one workgroup that sorts the k results.
 *                               k == 0 or col->n_vectors == 0: ALPGPU_OK and *d_count = 0 (that one write is still enqueued).
 *                               ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx, col, d_count, d_vals, d_mask or d_scratch;
 *                               k > ALPGPU_TOP_K_MAX; d_records or d_scratch not 16-byte aligned, d_mask, d_count or d_idx not 8-byte aligned,
 *                               d_vals not aligned to its type; n_vectors >= 2^32 or, with n_vectors > 0, a column without descriptors.
 *   alpgpu_top_k_scratch_bytes  the scratch of a call: caller-owned device memory, 16-byte aligned; what it holds before does not matter and what it
 *                               holds after is unspecified.  It covers the records and counts (20 bytes per vector, also when d_records is given:
 *                               one formula), min(k, n_vectors) * 1024 candidates of 16 bytes, ALPGPU_TOP_K_MAX staging slots, the histogram bins
 *                               and the device-side state.  Never 0, monotone in both arguments; UINT64_MAX for k > ALPGPU_TOP_K_MAX and for
 *                               n_vectors >= 2^32.
 * Contract as for the masked MIN / MAX section: everything is enqueued on the context's stream and on that stream only: asynchronous, no host
 *   synchronisation, no allocation; none of what the context remembers about columns is read or written; safe inside a stream capture (a replay
 *   sees the bitmap's, the records' and the column's contents of that time; k, largest and the pointers are fixed at capture).  All counts live in
 *   device memory, every grid is fixed on the host and no workgroup waits for another.  (tests/top_k_replica.py holds the host replica.)
 * TRUST: as for alpgpu_select_range_* (descriptors followed as found; exception positions ascend within a vector). */
#define ALPGPU_TOP_K_MAX 1024
uint64_t alpgpu_top_k_scratch_bytes(uint64_t n_vectors, uint64_t k);
int alpgpu_top_k_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f64* d_records, uint64_t k, int largest, double* d_vals, int64_t* d_idx,
                     uint64_t* d_count, void* d_scratch);
int alpgpu_top_k_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f32* d_records, uint64_t k, int largest, float* d_vals, int64_t* d_idx,
                     uint64_t* d_count, void* d_scratch);

/* ---- quantiles ---------------------------------------------------------------------------------------------------------------------------------
 * Exact order statistics under a WHERE clause: the median, percentiles, the r-th smallest selected value.  No value of the column reaches HBM but
 * candidate keys bounded by a capacity.
 *   PERCENTILE_DISC(q) WITHIN GROUP (ORDER BY x)   quantile(x, bitmap, q): the lower neighbour (q * (N - 1) floored; numpy's method="lower");
 *   PERCENTILE_CONT(q) ...                         the two neighbours, interpolated by the caller: lo + (hi - lo) * (q * (N - 1) - r);
 *   ORDER BY x LIMIT 1 OFFSET r                    select_rank(x, bitmap, {r}); ORDER BY x DESC: from_top = 1.
 * Let S be the values of the column at the set bits of the bitmap that are not NaNs (NaN by the bits, quiet or signalling, in an exception record
 * as in packed words), N = |S|, and s_0 <= s_1 <= ... <= s_{N-1} S sorted by okey ascending: top-k's order, -inf < ... < -0.0 < +0.0 < ... < +inf.
 * okey is a bijection on bits, so equal keys are equal bit patterns and every s_j is a bit pattern that alpgpu_decode_* writes somewhere.
 *   alpgpu_select_rank_*        *d_count = N.  For i < n_ranks, d_vals[i] = s_{min(ranks[i], N-1)}; with from_top != 0, s_{N-1-min(ranks[i], N-1)}.
 *                               Ranks may repeat and come in any order.  N == 0 writes the count and nothing else.
 *   alpgpu_quantile_*           r_i = min(N-1, (uint64_t)floor(q[i] * (double)(N-1))): one IEEE double multiplication, not fused with anything, then
 *                               floor, computed on the device (N exists only there).  d_vals[2i] = s_{r_i}, d_vals[2i+1] = s_{min(r_i + 1, N-1)},
 *                               d_ranks[i] = r_i (d_ranks may be NULL).  q stays double for float columns.  Interpolating between the two
 *                               neighbours is the caller's arithmetic.  A q[i] outside [0, 1] or NaN is ALPGPU_ERR_INVALID.  N == 0 writes the
 *                               count and nothing else.
 *                               `ranks` and `q` are HOST arrays: read before the call returns, they travel as kernel arguments (as lo / hi of
 *                               alpgpu_decode_group_sum_*), and a captured graph keeps them.
 *                               d_mask: a selection bitmap of col->n_vectors * 16 words, 8-byte aligned, required, read and never written.
 *                               d_zones (may be NULL; aligned to its records): any zone map whose records CONTAIN the true masked intervals of
 *                               the vectors: alpgpu_decode_minmax_masked_*, the unmasked alpgpu_zone_map_*, widened records.  This is the rule of
 *                               alpgpu_select_range_zoned_*, not top-k's stricter one: the records only prune (from the second pass on, a vector
 *                               whose record meets no interval still looked at costs 16 bytes), and such records change no output byte.  A record
 *                               with a NaN bound prunes nothing.  Records that do not contain the truth give unspecified values; even then
 *                               nothing is read or written out of bounds, at most the documented number of values is written, and the call
 *                               returns.
 *                               Cost: a radix select over okey with 8-bit digits, 8 passes for double and 4 for float.  A pass decodes the
 *                               column in registers and counts in LDS until the values that can still be an answer fit the candidate capacity,
 *                               max(65536, 16 * n_vectors) keys of 8 bytes (1/64 of the values); the next pass also writes those keys out and the
 *                               remaining passes read only them.  If the bitmap's set bits fit the capacity, the first pass does: ONE decode.
 *                               A full column of decimal data takes 2 decodes for one quantile and 4 for 16 of them, one of values that share
 *                               their leading bytes (ALP_RD) 4 (profiles/r20_quantile.txt).  Worst case: a constant column (or any answer shared
 *                               by more values than the capacity) never fits and takes all 8 (4) decodes.
 *                               col->n_vectors == 0: ALPGPU_OK and *d_count = 0 (that one write is still enqueued).
 *                               ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx, col, d_count, d_vals, d_mask, d_scratch, ranks or q;
 *                               n_ranks == 0 or > ALPGPU_RANK_MAX, n_q == 0 or > ALPGPU_QUANTILE_MAX; d_scratch not 16-byte aligned, d_mask, d_count
 *                               or d_ranks not 8-byte aligned, d_vals not aligned to its type, d_zones not aligned to its records; n_vectors >=
 *                               2^32 or, with n_vectors > 0, a column without descriptors.
 *   alpgpu_quantile_scratch_bytes  the scratch of a call: caller-owned device memory, 16-byte aligned; what it holds before does not matter and what it
 *                               holds after is unspecified (alpgpu_debug_quantile_trace reads it).  A function of n_vectors alone: the state, the bins
 *                               of 8 passes and the candidate keys.  Never 0, monotone; UINT64_MAX for n_vectors >= 2^32.
 * Contract as for the top-k section: everything is enqueued on the context's stream and on that stream only: asynchronous, no host synchronisation,
 *   no allocation; none of what the context remembers about columns is read or written; safe inside a stream capture (a replay sees the bitmap's,
 *   the records' and the column's contents of that time).  All counts live in device memory, every grid is fixed on the host and no workgroup waits
 *   for another.  Only integer atomics are used and keys are exact: the result is a function of the column, the bitmap and the ranks alone, not of
 *   launch shapes or of the order in which wavefronts arrive.  (tests/quantile_replica.py holds the host replica.)
 * TRUST: as for alpgpu_select_range_* (descriptors followed as found; exception positions ascend within a vector). */
#define ALPGPU_RANK_MAX     32
#define ALPGPU_QUANTILE_MAX 16
uint64_t alpgpu_quantile_scratch_bytes(uint64_t n_vectors);
int alpgpu_select_rank_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, const uint64_t* ranks, uint32_t n_ranks, int from_top,
                           double* d_vals, uint64_t* d_count, void* d_scratch);
int alpgpu_select_rank_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, const uint64_t* ranks, uint32_t n_ranks, int from_top,
                           float* d_vals, uint64_t* d_count, void* d_scratch);
int alpgpu_quantile_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, const double* q, uint32_t n_q, double* d_vals,
                        uint64_t* d_ranks, uint64_t* d_count, void* d_scratch);
int alpgpu_quantile_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, const double* q, uint32_t n_q, float* d_vals,
                        uint64_t* d_ranks, uint64_t* d_count, void* d_scratch);
/* debug / test: alpgpu_select_rank_* with a tuning record, so that small columns reach every path.  A 0 field means the default.  capacity: the candidate
 * keys, which may only be lowered (the scratch keeps its documented size; a larger value is the default); max_workgroups: of the decode passes' grid;
 * flush_every: trips of a workgroup's loop (8 vectors each) between two flushes of its LDS bins (default 2^18).  No tuning changes an output byte.
 * alpgpu_debug_quantile_trace: what the last call on this scratch did (any of the entry points above); synchronises the context's stream.  compact_pass:
 * the pass that wrote the candidates out, 0 .. passes - 1, or the number of passes (8 / 4) for never; candidates: keys appended; n: N; zone_skips[d]:
 * vectors skipped by their record in pass d; zero_skips: vectors skipped in the first pass for an all-zero bitmap; the decode passes' grid and
 * wavefronts per workgroup. */
typedef struct alpgpu_quantile_tuning {
    uint64_t capacity;
    uint32_t max_workgroups;
    uint32_t flush_every;
} alpgpu_quantile_tuning;
typedef struct alpgpu_quantile_trace {
    uint32_t compact_pass;
    uint32_t wide_grid;
    uint32_t waves_per_wg;
    uint32_t reserved;
    uint64_t candidates;
    uint64_t n;
    uint64_t zero_skips;
    uint64_t zone_skips[8];
} alpgpu_quantile_trace;
int alpgpu_debug_quantile_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, const uint64_t* ranks, uint32_t n_ranks,
                              int from_top, double* d_vals, uint64_t* d_count, void* d_scratch, const alpgpu_quantile_tuning* tuning);
int alpgpu_debug_quantile_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, const uint64_t* ranks, uint32_t n_ranks,
                              int from_top, float* d_vals, uint64_t* d_count, void* d_scratch, const alpgpu_quantile_tuning* tuning);
int alpgpu_debug_quantile_trace(alpgpu_ctx* ctx, const void* d_scratch, alpgpu_quantile_trace* out);

/* ---- histograms --------------------------------------------------------------------------------------------------------------------------------
 * The bucket counts of a column's selected values by sorted edges, no decoded value reaching HBM: width_bucket(x, ...) / GROUP BY bucket with
 * COUNT(*); COUNT(*) GROUP BY key for a dictionary-coded key with up to thousands of distinct values (point buckets: edges = the keys, bucket i + 1
 * counts key i); equi-width and equi-depth statistics; density plots.  One decode for up to 4096 buckets, where alpgpu_decode_group_sum_* with
 * counts serves 16 key ranges per call.
 *   alpgpu_histogram_*          Take every value index r of [first, first + n) whose bit is set in the bitmap (d_mask == NULL: every r of the range).
 *                               x_r is, bit for bit, what alpgpu_decode_* writes at r, exceptions patched in.
 *                                 x_r is a NaN (by the bits: quiet or signalling)   counts in d_counts[n_edges + 1];
 *                                 right == 0                                        counts in d_counts[b], b = #{i : d_edges[i] <= x_r}: the half-open
 *                                                                                   buckets [e[b-1], e[b]); numpy.searchsorted(side="right"),
 *                                                                                   torch.bucketize(right=True);
 *                                 right != 0                                        b = #{i : d_edges[i] < x_r}: the buckets (e[b-1], e[b]].
 *                               Bucket 0 lies below the first edge, bucket n_edges at or above the last.  The comparisons are C's: -0.0 == +0.0, and
 *                               +-inf are ordinary values and ordinary edges.  A NaN edge is never <= anything: NaNs sorted last are inert (the rule
 *                               alpgpu_select_in_mask_* states for its list).  n_edges == 0 is valid (d_edges may be NULL): one bucket and the NaN
 *                               counter, COUNT of the values that are no NaNs.
 *                               d_edges: n_edges elements of the column's type in DEVICE memory, aligned to the element, sorted as numpy.sort
 *                               sorts, read when the kernel runs (a captured graph sees the edges' contents at replay; n_edges and the pointers are
 *                               fixed at capture).  Duplicates are allowed and give empty buckets.  An array that is not sorted gives unspecified
 *                               bucket counts; nothing is read outside d_edges[0 .. n_edges) nor written outside d_counts[0 .. n_edges + 2), and the
 *                               sum over all n_edges + 2 words is still the number of selected values.  n_edges > ALPGPU_HISTOGRAM_EDGES_MAX
 *                               returns ALPGPU_ERR_INVALID: the edges sit whole in LDS, and a pivot tier for longer arrays (what
 *                               alpgpu_select_in_mask_* has for its list) is not built.
 *                               d_counts: n_edges + 2 words of 8 bytes.  accumulate == 0: the call overwrites them (they are zeroed on the context's
 *                               stream in front of the kernel; what they held does not matter).  accumulate != 0: the call adds to what they hold: shards
 *                               of one column on several GPUs after a copy, successive ranges, several columns into one histogram; exact in
 *                               every case.
 *                               d_mask (may be NULL): a selection bitmap of col->n_vectors * 16 words, 8-byte aligned, read and never written.  A
 *                               vector whose words are all zero within the range costs its 128 bytes and nothing of the column; one outside the
 *                               range costs nothing.
 *                               d_zones (may be NULL; aligned to its records): any zone map whose records CONTAIN the true intervals of the
 *                               vectors' selected values: alpgpu_zone_map_*, alpgpu_decode_minmax_masked_*, widened records.  Such records change no
 *                               count.  A vector whose record lies in ONE bucket, and whose descriptor says ALP without exceptions (a NaN in an ALP
 *                               vector is always an exception), is the popcount of its selected bits; its packed words are not read.  Any other
 *                               vector is decoded, its per-value search narrowed to the buckets its record admits.  A record with a NaN bound
 *                               prunes nothing.  Records that do not contain the truth give unspecified bucket counts; the total stays right and
 *                               nothing is read or written out of bounds.
 *                               Cost: the zeroing (a small kernel of the library's own, which a captured graph replays faithfully) and one
 *                               launch of persistent workgroups, sized to the device; a workgroup stages the edges into
 *                               LDS once and counts in 32-bit LDS bins, added into d_counts by 64-bit integer atomics at its end (and every 2^18
 *                               trips, so that no LDS bin overflows).  A value costs ceil(log2(n_edges + 1)) LDS probes and one LDS add; a step of
 *                               64 values that agree on their bucket costs one add.
 *                               col->n_vectors == 0: ALPGPU_OK, nothing is written.  n == 0: the counts are zeroed unless accumulate is set, and
 *                               nothing of the column is read.
 *                               ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx, col or d_counts; a NULL d_edges with n_edges > 0;
 *                               n_edges > ALPGPU_HISTOGRAM_EDGES_MAX; d_mask, d_counts or d_trace not 8-byte aligned, d_edges not aligned to its
 *                               elements, d_zones not aligned to its records; a range past the end; with n_vectors > 0 and n > 0, a column without
 *                               descriptors.
 * The call runs on the context's stream and on that stream only: asynchronous, no host synchronisation, no allocation, no scratch, no state kept; none
 *   of what the context remembers about columns (the decode plans) is read or written; safe inside a stream capture.  Only integer atomics are used
 *   and no workgroup waits for another: the counts are a function of the column, the bitmap, the edges and the arguments alone, not of launch shapes
 *   or of the order in which wavefronts arrive.  (tests/histogram_replica.py holds the host replica.)
 * TRUST: as for alpgpu_select_range_* (descriptors followed as found; exception positions ascend within a vector). */
#define ALPGPU_HISTOGRAM_EDGES_MAX 4095
int alpgpu_histogram_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, const double* d_edges,
                         uint32_t n_edges, int right, int accumulate, uint64_t* d_counts);
int alpgpu_histogram_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, const float* d_edges,
                         uint32_t n_edges, int right, int accumulate, uint64_t* d_counts);
/* debug / test: alpgpu_histogram_* with a tuning record, so that small columns reach every path, and a trace.  A 0 field means the default.  grid: the
 * workgroups launched (default min(ceil(n_vectors / 8), 3 per CU); more than the column has work for is allowed, at most 65536); flush_every: trips of
 * a workgroup's loop (8 vectors each) between two flushes of its LDS bins (default 2^18; may only be lowered).  No tuning changes a count.
 * d_trace (may be NULL): 4 words of device memory that the call ADDS to, each wavefront once per word at its end: vectors
 *   [0] settled without the column (their bitmap words are all zero within the range, or they lie outside the range),
 *   [1] settled from their zone record,
 *   [2] settled by a few-bucket route: always 0; that route is not in the library ("Histograms"),
 *   [3] decoded. */
typedef struct alpgpu_histogram_tuning {
    uint32_t grid;
    uint32_t flush_every;
} alpgpu_histogram_tuning;
int alpgpu_debug_histogram_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, const double* d_edges,
                               uint32_t n_edges, int right, int accumulate, uint64_t* d_counts, const alpgpu_histogram_tuning* tuning, uint64_t* d_trace);
int alpgpu_debug_histogram_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, const float* d_edges,
                               uint32_t n_edges, int right, int accumulate, uint64_t* d_counts, const alpgpu_histogram_tuning* tuning, uint64_t* d_trace);

/* ---- join probe ---------------------------------------------------------------------------------------------------------------------------------
 * Which build-side row does each probe row match: the selected values of a compressed column (a foreign key) looked up in a sorted key list (the
 * build side: a filtered dimension's keys, what alpgpu_decode_masked_* hands back, sorted), no decoded value reaching HBM.  alpgpu_select_in_mask_*
 * answers WHETHER x is a key (a semi-join); this call keeps the position its lower bound found.  The two routes it completes (TPC-H Q3, Q5, Q10:
 * lineitem x orders x customer, a foreign key looked up in a filtered dimension):
 *   inner join        select_in_mask(fk, keys, AND) on the bitmap; join_probe(fk, bitmap, keys, rows) -> d_pos; gather(dim_col, d_pos): no row is NO_MATCH.
 *   left outer join   join_probe alone; alpgpu_gather_* turns the index -1 into the canonical NaN, the NULL of the outer side.
 *   alpgpu_join_probe_*         One output row per set bit of d_mask, in ascending value index: rows, order and capacity are exactly those of
 *                               alpgpu_decode_masked_*.  *d_count = the number of set bits, also when it exceeds `capacity`; rows j <
 *                               min(*d_count, capacity) are written, nothing at or behind `capacity` and nothing at j >= *d_count.  capacity == 0
 *                               makes the call a count: d_pos, d_span and d_idx may then be NULL.  d_idx (may be NULL): the value index of row j,
 *                               bit for bit what alpgpu_mask_to_indices writes.
 *                               d_mask == NULL means every one of the n_vectors * 1024 indices: row j is index j, d_scratch may be NULL, no count
 *                               or scan launch is made, and *d_count = n_vectors * 1024 is still written, by a kernel (not by a memset node, which
 *                               a captured graph was seen to replay wrongly: DESIGN.md, "Histograms").  With a bitmap (n_vectors * 16 words, 8-byte
 *                               aligned, read and never written) d_scratch is alpgpu_select_scratch_bytes(n_vectors) bytes, 16-byte aligned, in
 *                               the selection's layout: the popcount pass and the scan are those of alpgpu_decode_masked_*.
 *                               The match.  x = the value at row j's index, bit for bit what alpgpu_decode_* writes there, exceptions patched in.
 *                               lb = the number of keys < x, ub = the number of keys <= x.
 *                                 d_span[j] (d_span may be NULL) = ub - lb: the number of keys == x under C's ==.  -0.0 and +0.0 match each other,
 *                                                                a NaN value never matches and neither does a NaN key, +-inf are ordinary.
 *                                 d_pos[j]   no match (ub == lb)          ALPGPU_JOIN_NO_MATCH;
 *                                            match, d_rows == NULL        lb: the position of the first equal key;
 *                                            match, d_rows given          d_rows[lb]: the payload stored beside the keys, e.g. torch.sort's `indices`,
 *                                                                         so that the caller has build-side row ids without a second indexing pass.
 *                               d_rows (n_keys words of 8 bytes, 8-byte aligned) is read only at matched positions.  The equal run is [lb, lb + span)
 *                               in d_keys, and in d_rows: all an N:M expansion needs.  The upper bound is searched only when d_span is given.
 *                               d_keys: n_keys elements of the column's type in DEVICE memory, aligned to the element, read when the kernel runs (a
 *                               captured graph sees the keys' contents at replay; n_keys and the pointers are fixed at capture), sorted by the
 *                               rules of alpgpu_select_in_mask_*'s list: as numpy.sort sorts, -0.0 and +0.0 in either order, duplicates allowed,
 *                               NaNs, if any, last.  n_keys == 0 is valid (d_keys may be NULL): nothing matches.  n_keys > 2^31 - 1 returns
 *                               ALPGPU_ERR_INVALID.
 *                               d_zones (may be NULL): the column's zone map, by the contract of alpgpu_select_in_mask_*.  A vector whose
 *                               [min, max] admits no key gets ALPGPU_JOIN_NO_MATCH and span 0 at all of its set bits; its descriptor, packed words
 *                               and exception record are not read.  For every other vector the search is narrowed to the part [j0, j1) of the keys
 *                               that the record admits.  Any zone map that contains the vectors' true intervals gives the bytes of the call without
 *                               zones; a NaN bound means "decode the vector".
 *                               Robustness.  Keys that are not sorted, or a zone map that lies, change only d_pos and d_span: every d_pos is then
 *                               ALPGPU_JOIN_NO_MATCH, or lies in [0, n_keys), or is an element of d_rows[0 .. n_keys); every span is <= n_keys;
 *                               *d_count and d_idx are unaffected; nothing is read outside d_keys, d_rows or the column and nothing is written
 *                               outside the first min(count, capacity) rows: every probe index is clamped.
 *                               Cost: with a bitmap the popcount pass and the scan; then one launch of persistent workgroups, sized to the device
 *                               and not to the column.  A workgroup stages the keys into LDS once, as alpgpu_select_in_mask_* does its list (whole
 *                               up to alpgpu_in_list_lds_max(value bytes) elements, every stride-th beyond); a value costs the probes of one
 *                               search (two with d_span) and one ==.  A vector without a set bit costs 4 bytes, one behind the capacity 12; the
 *                               packed words and exception values are read only for the quarters of a vector that hold a bit.
 *                               col->n_vectors == 0: *d_count = 0 is written and nothing else.
 *                               ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx, col or d_count; a NULL d_pos with capacity > 0; a NULL
 *                               d_scratch (or one not 16-byte aligned) with a bitmap and n_vectors > 0; a NULL d_keys with n_keys > 0;
 *                               n_keys > 2^31 - 1; d_mask, d_rows, d_pos, d_idx or d_count not 8-byte aligned, d_span not 4-byte aligned, d_keys
 *                               not aligned to its elements, d_zones not aligned to its records; with n_vectors > 0 and capacity > 0, a column
 *                               without descriptors.
 * The call runs on the context's stream and on that stream only: asynchronous, no host synchronisation, no allocation, no state kept, no atomics on
 *   results (none at all); none of what the context remembers about columns (the decode plans) is read or written; safe inside a stream capture.
 *   The result is a function of the column, the bitmap, the keys, the rows and the arguments alone.  (tests/join_replica.py holds the host replica.)
 * TRUST: as for alpgpu_select_range_* (descriptors followed as found; exception positions ascend within a vector). */
#define ALPGPU_JOIN_NO_MATCH (-1)
int alpgpu_join_probe_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, const double* d_keys, uint64_t n_keys,
                          const int64_t* d_rows, int64_t* d_pos, uint32_t* d_span, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch);
int alpgpu_join_probe_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, const float* d_keys, uint64_t n_keys,
                          const int64_t* d_rows, int64_t* d_pos, uint32_t* d_span, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch);

/* ---- distinct values ------------------------------------------------------------------------------------------------------------------------------
 * The sorted distinct values of a column's selected values and how often each occurs, no decoded value reaching HBM: SELECT DISTINCT x,
 * COUNT(DISTINCT x), value_counts, GROUP BY key with COUNT(*) when the keys are NOT known in advance.  The output is directly a valid edge array for
 * alpgpu_histogram_* (point buckets), a valid list for alpgpu_select_in_mask_* and a valid key array for alpgpu_join_probe_*: the call that feeds
 * the three without a decode, a sort and a unique outside the library.
 *   alpgpu_distinct_*           Take every value index r of [first, first + n) whose bit is set in the bitmap (d_mask == NULL: every r of the range).
 *                               x_r is, bit for bit, what alpgpu_decode_* writes at r, exceptions patched in.
 *                               NaNs.  A NaN (by the bits: quiet or signalling, packed or an exception) is never a distinct value: NaNs are only
 *                               counted, in d_state[1].
 *                               Equality is C's ==, as for alpgpu_select_in_mask_*, alpgpu_histogram_* and alpgpu_join_probe_*: -0.0 and +0.0 are ONE
 *                               value, reported as +0.0; +-inf are ordinary values.  (A zero is made +0.0 before the order key okey of "top-k" is
 *                               taken; from there on equal values are equal bit patterns and everything is integer.)
 *                               Output.  Let u_0 < u_1 < ... < u_{D-1} be the distinct values, ascending.  With D <= capacity:
 *                                 d_vals[i]   = u_i, i < D;
 *                                 d_counts[i] (d_counts may be NULL) = the number of selected r with x_r == u_i.
 *                               Nothing is written at d_vals[D ...] or d_counts[D ...].
 *                               d_state: 4 words of 8 bytes, always written (also for n == 0 and for a column of no vectors):
 *                                 [0] the number of entries written, min(D, capacity);
 *                                 [1] the selected NaNs;
 *                                 [2] the selected values that are no NaNs, counted by popcounts beside the table: right also on overflow;
 *                                 [3] 1 if D > capacity (overflow), else 0.
 *                               Without overflow the sum of d_counts[0 .. D) is d_state[2].  On overflow the contents of d_vals and
 *                               d_counts[0 .. capacity) are unspecified; nothing is ever written at or beyond `capacity`, and the call returns as
 *                               always: call again with a larger capacity.
 *                               capacity: 1 .. ALPGPU_DISTINCT_MAX.  d_scratch: alpgpu_distinct_scratch_bytes(capacity) bytes, 16-byte aligned,
 *                               contents irrelevant before and unspecified after; one formula (T = the power of two >= 2 * capacity, P = the power
 *                               of two >= capacity): 64 bytes of state, T keys and T counts of 8 bytes (the table), P pairs of 16 bytes (the sort).
 *                               d_mask (may be NULL): a selection bitmap of col->n_vectors * 16 words, 8-byte aligned, read and never written.  A
 *                               vector whose words are all zero within the range costs its 128 bytes and nothing of the column; one outside the
 *                               range costs nothing.
 *                               d_zones (may be NULL; aligned to its records): any zone map whose records CONTAIN the true intervals of the
 *                               vectors' selected values (alpgpu_histogram_*'s rule): alpgpu_zone_map_*, alpgpu_decode_minmax_masked_*, widened
 *                               records.  ONE shortcut is taken: a record with min == max (neither a NaN) on a vector whose descriptor says ALP
 *                               without exceptions (a NaN in an ALP vector is always an exception) is one insert of that value with the popcount of
 *                               the vector's selected bits; its packed words are not requested.  Every other vector is decoded.  Truthful records
 *                               change no output byte.  Records that do not contain the truth give unspecified values and counts; d_state[1] +
 *                               d_state[2] is still the number of selected values and nothing is read or written out of bounds.
 *                               Cost: a reset kernel (the table to EMPTY = all-ones, the order key of a NaN pattern, which is never inserted; not a
 *                               memset node: DESIGN.md, "Histograms"); one launch of persistent workgroups, sized to the device, that decode in
 *                               registers and insert into an open-addressing table in LDS (a step of 64 values that agree on their value costs one
 *                               insert) which is flushed into the global table (multiplicative hash, linear probing, integer atomics) at the
 *                               workgroup's end and every 2^18 trips; a compaction of the occupied slots; a bitonic sort of the at most `capacity`
 *                               (key, count) pairs, whose launch count depends on `capacity` alone; the emit.  Every probe loop is bounded by the
 *                               slots of the table it walks and no workgroup waits for another.  A low-cardinality column costs about one
 *                               histogram; near 2^20 distinct values the random global atomics dominate.
 *                               n == 0: a zero state is written and nothing of the column is read.  col->n_vectors == 0: ALPGPU_OK, the zero state
 *                               is written.
 *                               ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx, col, d_vals, d_state or d_scratch; capacity == 0 or
 *                               beyond ALPGPU_DISTINCT_MAX; d_scratch not 16-byte aligned; d_mask, d_counts, d_state or d_trace not 8-byte aligned,
 *                               d_vals not aligned to its elements, d_zones not aligned to its records; a range past the end; with n_vectors > 0 and
 *                               n > 0, a column without descriptors.
 *   alpgpu_distinct_scratch_bytes   the formula above: never 0, monotone in capacity, a multiple of 16; UINT64_MAX for capacity == 0 or beyond
 *                               ALPGPU_DISTINCT_MAX.
 * The call runs on the context's stream and on that stream only: asynchronous, no host synchronisation, no allocation, no state kept; none of what
 *   the context remembers about columns (the decode plans) is read or written; safe inside a stream capture (a replay sees the bitmap's and the
 *   column's contents of that time).  Every grid is fixed on the host, all counts live in device memory and only integer atomics are used: the result
 *   is a function of the column, the bitmap and the arguments alone, not of launch shapes or of the order in which wavefronts arrive.
 *   (tests/distinct_replica.py holds the host replica.)
 * Not built: distinct by bit pattern (the zeros apart), more than 2^20 distinct values, a multi-column DISTINCT, zone pruning beyond the
 *   constant-vector rule.
 * TRUST: as for alpgpu_select_range_* (descriptors followed as found; exception positions ascend within a vector). */
#define ALPGPU_DISTINCT_MAX (1u << 20)
uint64_t alpgpu_distinct_scratch_bytes(uint64_t capacity);
int alpgpu_distinct_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, uint64_t capacity,
                        double* d_vals, uint64_t* d_counts, uint64_t* d_state, void* d_scratch);
int alpgpu_distinct_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, uint64_t capacity,
                        float* d_vals, uint64_t* d_counts, uint64_t* d_state, void* d_scratch);
/* debug / test: alpgpu_distinct_* with a tuning record, so that small columns reach every path, and a trace.  A 0 field means the default; no field
 * changes an output byte.  grid: the workgroups of the insert launch (default min(ceil(vectors of the range / 8), 3 per CU for float and 2 for double);
 * more than there is work for is allowed, at most 65536).  flush_every: trips of a workgroup's loop (8 vectors each) between two flushes of its LDS table (default 2^18; may
 * only be lowered).  lds_slots: slots of the workgroup's LDS table (default 4096; a power of two, may only be lowered, at least 64; other values are
 * rounded down to a power of two).  table_slots: slots of the global table (default T; may be lowered down to P, the power of two at or above
 * `capacity`, so that a full table and wrapped probes are reached with small inputs).  sort_tile: pairs sorted in LDS by one workgroup (default 4096;
 * a power of two, may only be lowered, at least 64), so that a few hundred distinct values reach the multi-launch part of the sort.
 * d_trace (may be NULL): 6 words of device memory that the call ADDS to:
 *   [0] vectors of the range settled without the column (their selected bits are all zero),
 *   [1] vectors settled from their zone record,
 *   [2] vectors decoded,
 *   [3] steps (64 values) settled by wave agreement: one insert,
 *   [4] inserts offered to the LDS table (one per agreeing step or settled vector, one per selected value otherwise),
 *   [5] inserts made into the global table (direct ones plus flushed LDS entries). */
typedef struct alpgpu_distinct_tuning {
    uint32_t grid;
    uint32_t flush_every;
    uint32_t lds_slots;
    uint32_t table_slots;
    uint32_t sort_tile;
    uint32_t reserved;
} alpgpu_distinct_tuning;
int alpgpu_debug_distinct_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, uint64_t capacity,
                              double* d_vals, uint64_t* d_counts, uint64_t* d_state, void* d_scratch, const alpgpu_distinct_tuning* tuning, uint64_t* d_trace);
int alpgpu_debug_distinct_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, uint64_t capacity,
                              float* d_vals, uint64_t* d_counts, uint64_t* d_state, void* d_scratch, const alpgpu_distinct_tuning* tuning, uint64_t* d_trace);

/* ---- keyed aggregation ----------------------------------------------------------------------------------------------------------------------------
 * SELECT key, SUM(x), COUNT(*) ... WHERE ... GROUP BY key for up to 1024 discrete keys known in advance (alpgpu_distinct_* hands them over sorted),
 * in ONE pass that decodes both columns in registers, no decoded value reaching HBM.  alpgpu_decode_group_sum_* stays the call for up to 16 RANGE
 * groups with per-vector rows; alpgpu_histogram_* with point buckets is the COUNT(*) alone.
 *   alpgpu_decode_keyed_sum_*   (built for double columns: _f64.)  val and key: two columns of the entry point's type with equal n_vectors; val == key is allowed.  Take every row r
 *                               whose bit is set in the bitmap (d_mask == NULL: every row).  x_r and k_r are, bit for bit, what alpgpu_decode_* writes
 *                               at r for val and for key, exceptions patched in; a float x_r is widened to double first (exactly).
 *                               d_keys: n_keys elements of the key column's type in DEVICE memory, aligned to the element, sorted as numpy.sort
 *                               sorts, read when the kernel runs (a captured graph sees the keys' contents at replay; n_keys and the pointers are
 *                               fixed at capture), as alpgpu_select_in_mask_* reads its list.  n_keys is 1 .. ALPGPU_KEYED_KEYS_MAX: the keys and
 *                               every wavefront's private table of them sit in LDS; more keys means calling again with the next 1024.
 *                               The match.  Row r belongs to key i if i is the FIRST position with d_keys[i] == k_r: the lower bound of
 *                               alpgpu_select_in_mask_* and one C ==.  -0.0 matches +0.0; a NaN k_r matches nothing and a NaN in d_keys (sorted
 *                               last) is never matched; later duplicates in d_keys receive +0.0 and 0.  A selected row that matches no key is
 *                               counted in d_counts[n_keys].
 *                               d_counts (may be NULL): n_keys + 1 words of 8 bytes, exact integers.  With sorted keys and records that do not lie,
 *                               the sum of all n_keys + 1 words is the number of selected rows.
 *                               d_sums: n_keys doubles, in THIS order and no other.  Let L = alpgpu_keyed_stripe_vectors(n_vectors); stripe s is
 *                               the vectors [s L, min((s + 1) L, n_vectors)), S = ceil(n_vectors / L) of them.  For key i, vector v and step
 *                               m = 0..15, P(i, v, m) is the adjacent-lane tree of alpgpu_decode_sum_* over 64 lanes — (0,1), (2,3), ...; six
 *                               levels — where lane l holds x at row 1024 v + 64 m + l if that row is selected and belongs to key i, else +0.0.
 *                               The stripe's partial A(i, s) starts at +0.0 and takes += P(i, v, m) for v ascending within the stripe and, within
 *                               a vector, m ascending.  (A step in which no lane belongs to i may be left out: adding +0.0 changes no accumulator
 *                               that began at +0.0, whose sums are never -0.0.)  d_sums[i] is, bit for bit, alpgpu_tree_sum_f64 over
 *                               A(i, 0 .. S).  A selected NaN in val makes its key's sum a NaN of unspecified payload.  Neither the grid, nor the
 *                               device's CU count, nor the order in which wavefronts arrive enters the result: a stripe's partial is the work
 *                               of one wavefront, whichever takes it.  (tests/keyed_replica.py holds the host replica.)
 *                               d_mask (may be NULL): a selection bitmap of n_vectors * 16 words, 8-byte aligned, read and never written.  A vector
 *                               whose 16 words are zero costs its 128 bytes and nothing of either column.
 *                               d_key_zones (may be NULL; aligned to its records): any zone map whose records CONTAIN the true intervals of the
 *                               KEY vectors' selected values (alpgpu_histogram_*'s rule).  A record narrows its vector's search to the keys it
 *                               admits; a vector whose record admits no key is rows without a key, and neither column is read.  A record with
 *                               min == max (neither a NaN) on a key vector whose descriptor says ALP without exceptions settles the key of every
 *                               selected row: the key vector's packed words are not requested, only the value vector is decoded.  A record with a
 *                               NaN bound prunes nothing.  Truthful records change no bit.  Records that do not contain the truth, or keys that
 *                               are not sorted, give unspecified sums and counts; the sum of the n_keys + 1 counts is still the number of selected
 *                               rows, and nothing is read outside d_keys[0 .. n_keys) or the columns nor written outside the outputs: every probe
 *                               index is clamped.
 *                               d_scratch: alpgpu_keyed_sum_scratch_bytes(n_vectors, n_keys) bytes, 16-byte aligned, contents irrelevant before
 *                               and unspecified after: 64 bytes of header (the stripe ticket) and the stripe partials, S rows of n_keys doubles.
 *                               Cost: an init kernel (the counts and the ticket zeroed; not a memset node: DESIGN.md, "Histograms"), one launch of
 *                               persistent workgroups sized to the device, whose wavefronts take stripes by an integer ticket and keep a private
 *                               table of n_keys doubles and 32-bit counts in LDS (two capacity tiers: up to 256 keys and up to 1024), and a
 *                               reduce of one small workgroup per key.  A value costs ceil(log2(n_keys + 1)) LDS probes; a step of 64 rows that
 *                               agree on their key costs one tree and one LDS add, a row alone with its key in its step one LDS add.
 *                               n_vectors == 0: every sum is +0.0 and every count 0, written by a kernel; neither column is read.
 *                               ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx, val, key, d_keys, d_sums or d_scratch; n_keys outside
 *                               1 .. ALPGPU_KEYED_KEYS_MAX; columns that differ in n_vectors; n_vectors > 2^32 - 1; d_scratch not 16-byte aligned;
 *                               d_sums, d_counts, d_mask or d_trace not 8-byte aligned; d_keys not aligned to its elements, d_key_zones not aligned
 *                               to its records; with n_vectors > 0, a column without descriptors.
 *   alpgpu_keyed_stripe_vectors L = max(1, ceil(n_vectors / ALPGPU_KEYED_STRIPES_MAX)); host only.
 *   alpgpu_keyed_sum_scratch_bytes   64 + 8 * n_keys * min(n_vectors, ALPGPU_KEYED_STRIPES_MAX), rounded up to a multiple of 16: never less than the S
 *                               rows need, monotone in both arguments, at most 64 + 8 * n_keys * 4096; UINT64_MAX for n_keys outside 1 .. ALPGPU_KEYED_KEYS_MAX.
 * The call runs on the context's stream and on that stream only: asynchronous, no host synchronisation, no allocation, no state kept; none of what
 *   the context remembers about columns (the decode plans) is read or written; safe inside a stream capture.  No floating-point atomics; integer
 *   atomics for the counts and the ticket only; no workgroup waits for another.
 * Not built: more than 1024 keys per call (in this order; alpgpu_decode_keyed_exact_sum_* takes up to 2^20 keys and float columns, under its own
 *   contract), range groups (alpgpu_decode_group_sum_*), multi-column keys, keys not known in advance (alpgpu_distinct_* first).
 * TRUST: as for alpgpu_select_range_* (descriptors followed as found; exception positions ascend within a vector). */
#define ALPGPU_KEYED_KEYS_MAX    1024u
#define ALPGPU_KEYED_STRIPES_MAX 4096u
uint64_t alpgpu_keyed_stripe_vectors(uint64_t n_vectors);
uint64_t alpgpu_keyed_sum_scratch_bytes(uint64_t n_vectors, uint32_t n_keys);
int alpgpu_decode_keyed_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones, const double* d_keys,
                                uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_scratch);
/* (alpgpu_decode_keyed_sum_f32 is NOT built yet: double columns only.  The kernels are templates over the value width, but the float
 * instantiations have not been run on a 1 Mi-vector column and are left out until they have; DESIGN.md, "Keyed aggregation".) */
/* debug / test: alpgpu_decode_keyed_sum_* with a tuning record and a trace.  A 0 field means the default.  grid: the workgroups launched (default
 * min(ceil(S / wavefronts per workgroup), what the device holds); more than there is work for is allowed, at most 65536).  No tuning changes a bit.
 * d_trace (may be NULL): 4 words of device memory that the call ADDS to, each wavefront once per word at its end: vectors
 *   [0] settled without either column (their bitmap words are all zero),
 *   [1] settled by the constant-key shortcut (the key vector's packed words not requested),
 *   [2] whose zone record admits no key (rows without a key; neither column read),
 *   [3] decoded, both columns. */
typedef struct alpgpu_keyed_tuning {
    uint32_t grid;
    uint32_t reserved;
} alpgpu_keyed_tuning;
int alpgpu_debug_decode_keyed_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                      const double* d_keys, uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_scratch, const alpgpu_keyed_tuning* tuning,
                                      uint64_t* d_trace);

/* ---- keyed MIN / MAX ------------------------------------------------------------------------------------------------------------------------------
 * SELECT key, MIN(x), MAX(x), COUNT(*) ... WHERE ... GROUP BY key for up to 1024 discrete keys known in advance, in ONE pass that decodes both
 * columns in registers.  Built for double and float columns.
 *   alpgpu_decode_keyed_minmax_*   val, key (val == key allowed), d_mask, d_key_zones, d_keys and n_keys (1 .. ALPGPU_KEYED_KEYS_MAX) are
 *                               alpgpu_decode_keyed_sum_*'s, word for word, and so is the match: row r belongs to key i if i is the FIRST position
 *                               with d_keys[i] == k_r; -0.0 matches +0.0; a NaN k_r matches nothing and a NaN in d_keys is never matched; later
 *                               duplicates in d_keys receive nothing.  The zone-record rules are the same too: a record narrows its vector's
 *                               search; a record that admits no key means rows without a key, neither column read; min == max on a key vector
 *                               that is ALP without exceptions settles the key of every selected row without the key vector's packed words.
 *                               d_out: n_keys records {min, max} of the columns' type, aligned to the record (16 / 8 bytes).  Record i covers the
 *                               selected rows of val that belong to key i, in alpgpu_decode_minmax_masked_*'s order: NaNs ignored, -0.0 < +0.0,
 *                               +-inf ordinary values.  A key with no row, or whose rows hold only NaNs, and every later duplicate get
 *                               {+inf, -inf}.
 *                               d_counts (may be NULL): n_keys + 1 words of 8 bytes.  d_counts[i] counts every selected row of key i, NaN values
 *                               included (as alpgpu_decode_group_minmax_* counts them); the last word the selected rows without a key.  They are
 *                               alpgpu_decode_keyed_sum_*'s counts.
 *                               The equivalence: record i of a key that is the first of its equals is, bit for bit, alpgpu_group_minmax_totals_*
 *                               of row g of alpgpu_decode_group_minmax_* with lo[g] = hi[g] = d_keys[i] under the same bitmap.
 *                               Minimum and maximum are exact and order-free: records and counts are a function of the inputs alone; neither
 *                               the grid, nor the device's CU count, nor the order in which wavefronts arrive enters them.
 *                               Truthful zone records change no byte.  Records that do not contain the truth, or keys that are not sorted, give
 *                               unspecified records and counts; the sum of the n_keys + 1 counts is still the number of selected rows, and
 *                               nothing is read outside d_keys[0 .. n_keys) or the columns nor written outside the outputs: every probe index
 *                               is clamped.
 *                               Cost: an init kernel ({+inf, -inf} and 0; not a memset node: DESIGN.md, "Histograms") and one launch of persistent
 *                               workgroups sized to the device.  A workgroup keeps ONE table (mn, mx, 32-bit counts) and the keys in LDS, shared
 *                               by its wavefronts and updated by LDS integer atomics on the value bits, and joins it into d_out / d_counts at its
 *                               end by global integer atomics.  No scratch, no reduce kernel, no floating-point atomics.
 *                               n_vectors == 0: every record is {+inf, -inf} and every count 0, written by a kernel; neither column is read.
 *                               ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx, val, key, d_keys or d_out; n_keys outside
 *                               1 .. ALPGPU_KEYED_KEYS_MAX; columns that differ in n_vectors; n_vectors > 2^32 - 1; d_counts, d_mask or d_trace
 *                               not 8-byte aligned; d_out or d_key_zones not aligned to their records, d_keys not aligned to its elements; with
 *                               n_vectors > 0, a column without descriptors.
 * The call runs on the context's stream and on that stream only: asynchronous, no host synchronisation, no allocation, no state kept; safe inside a
 *   stream capture (the keys and the bitmap are read at replay).  No workgroup waits for another.
 * The debug entry takes alpgpu_keyed_tuning (grid) and adds to the four trace words of alpgpu_debug_decode_keyed_sum_*; no tuning changes a byte.
 * More than 1024 keys per call: alpgpu_decode_keyed_minmax_many_* (below), up to 2^20.
 * Not built: range groups (alpgpu_decode_group_minmax_*), multi-column keys, keys not known in advance.
 * TRUST: as for alpgpu_select_range_*. */
int alpgpu_decode_keyed_minmax_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                   const double* d_keys, uint32_t n_keys, alpgpu_zone_f64* d_out, uint64_t* d_counts);
int alpgpu_decode_keyed_minmax_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                   const float* d_keys, uint32_t n_keys, alpgpu_zone_f32* d_out, uint64_t* d_counts);
int alpgpu_debug_decode_keyed_minmax_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                         const double* d_keys, uint32_t n_keys, alpgpu_zone_f64* d_out, uint64_t* d_counts, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);
int alpgpu_debug_decode_keyed_minmax_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                         const float* d_keys, uint32_t n_keys, alpgpu_zone_f32* d_out, uint64_t* d_counts, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);

/* ---- keyed MIN / MAX, many keys -------------------------------------------------------------------------------------------------------------------
 * SELECT key, MIN(x), MAX(x), COUNT(*) ... WHERE ... GROUP BY key for up to 2^20 discrete keys known in advance, in ONE pass that decodes both
 * columns in registers: alpgpu_decode_keyed_minmax_* without its limit of 1024 keys, the table in device memory and not in LDS.  Built for double
 * and float columns.  alpgpu_distinct_* hands over up to ALPGPU_DISTINCT_MAX sorted keys; on the same selection it hands over their counts as well,
 * so d_counts == NULL is the usual call behind it.
 *   alpgpu_decode_keyed_minmax_many_*   val and key: two columns of the entry point's type with equal n_vectors; val == key is allowed.  Take every
 *                               row r whose bit is set in the bitmap (d_mask == NULL: every row).  x_r and k_r are, bit for bit, what
 *                               alpgpu_decode_* writes at r for val and for key, exceptions patched in.
 *                               d_keys: n_keys elements of the columns' type in DEVICE memory, aligned to the element, sorted as numpy.sort
 *                               sorts, read when the kernel runs (a captured graph sees the keys' contents at replay; n_keys and the pointers
 *                               are fixed at capture).  n_keys is 1 .. ALPGPU_KEYED_MANY_KEYS_MAX.
 *                               The match.  Row r belongs to key i if i is the FIRST position with d_keys[i] == k_r: the lower bound of
 *                               alpgpu_select_in_mask_* and one C ==.  -0.0 matches +0.0; a NaN k_r matches nothing and a NaN in d_keys (sorted
 *                               last) is never matched; later duplicates in d_keys receive nothing.  A selected row that matches no key is
 *                               counted in d_counts[n_keys].
 *                               d_out: n_keys records {min, max} of the columns' type, aligned to the record (16 / 8 bytes).  Record i covers the
 *                               selected rows of val that belong to key i, in alpgpu_decode_minmax_masked_*'s order: NaNs ignored, -0.0 < +0.0,
 *                               +-inf ordinary values.  A key with no row, or whose rows hold only NaNs, and every later duplicate get
 *                               {+inf, -inf}.
 *                               d_counts (may be NULL): n_keys + 1 words of 8 bytes.  d_counts[i] counts every selected row of key i, NaN values
 *                               included; the last word the selected rows without a key.  With d_counts == NULL no count is kept at all.
 *                               For n_keys <= ALPGPU_KEYED_KEYS_MAX records and counts are, byte for byte, those of
 *                               alpgpu_decode_keyed_minmax_* on the same arguments.
 *                               Minimum and maximum are exact and order-free: records and counts are a function of the inputs alone; neither
 *                               the grid, nor the device's CU count, nor the order in which wavefronts arrive enters them.
 *                               d_mask (may be NULL): a selection bitmap of n_vectors * 16 words, 8-byte aligned, read and never written.  A vector
 *                               whose 16 words are zero costs its 128 bytes and nothing of either column.
 *                               d_key_zones (may be NULL; aligned to its records): any zone map whose records CONTAIN the true intervals of the
 *                               KEY vectors' selected values.  A record narrows its vector's search to the keys it admits; a vector whose record
 *                               admits no key is rows without a key, and neither column is read.  A record with min == max (neither a NaN) on a
 *                               key vector whose descriptor says ALP without exceptions settles the key of every selected row: the key vector's
 *                               packed words are not requested, only the value vector is decoded.  A record with a NaN bound prunes nothing.
 *                               Truthful records change no byte.  Records that do not contain the truth, or keys that are not sorted, give
 *                               unspecified records and counts; the sum of the n_keys + 1 counts is still the number of selected rows, and
 *                               nothing is read outside d_keys[0 .. n_keys) or the columns nor written outside the outputs: every probe index
 *                               is clamped.
 *                               Cost: an init kernel ({+inf, -inf} and 0; not a memset node: DESIGN.md, "Histograms") and one launch of persistent
 *                               workgroups sized to the device.  A workgroup stages the keys into 32 KiB of LDS: up to 4096 doubles / 8192 floats
 *                               whole; of a longer list every stride-th key, and a value's search then ends in the list itself, between two of
 *                               those, ceil(log2(stride)) reads that L2 serves.  The table is d_out and d_counts: a matched row reads its key's
 *                               record and issues a global integer atomic on the value bits only where it improves on what it read; with
 *                               d_counts it adds one 64-bit integer atomic per row (one per step of 64 rows that agree on their key).  No
 *                               scratch, no reduce kernel, no floating-point atomics, no compare-and-swap loop.
 *                               n_vectors == 0: every record is {+inf, -inf} and every count 0, written by a kernel; neither column is read.
 *                               ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx, val, key, d_keys or d_out; n_keys outside
 *                               1 .. ALPGPU_KEYED_MANY_KEYS_MAX; columns that differ in n_vectors; n_vectors > 2^32 - 1; d_counts, d_mask or
 *                               d_trace not 8-byte aligned; d_out or d_key_zones not aligned to their records, d_keys not aligned to its
 *                               elements; with n_vectors > 0, a column without descriptors.
 * The call runs on the context's stream and on that stream only: asynchronous, no host synchronisation, no allocation, no state kept; safe inside a
 *   stream capture (the keys and the bitmap are read at replay).  No workgroup waits for another.
 * The debug entry takes alpgpu_keyed_tuning (grid) and adds to the four trace words of alpgpu_debug_decode_keyed_sum_*; no tuning changes a byte.
 * Not built: more than 2^20 keys per call, a keyed SUM beyond 1024 keys in alpgpu_decode_keyed_sum_*'s striped order (the route beyond is
 *   alpgpu_decode_keyed_exact_sum_*, below: another, stronger contract), range groups (alpgpu_decode_group_minmax_*), multi-column keys, keys not
 *   known in advance (alpgpu_distinct_* first).
 * TRUST: as for alpgpu_select_range_*. */
#define ALPGPU_KEYED_MANY_KEYS_MAX (1u << 20) /* == ALPGPU_DISTINCT_MAX */
int alpgpu_decode_keyed_minmax_many_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                        const double* d_keys, uint32_t n_keys, alpgpu_zone_f64* d_out, uint64_t* d_counts);
int alpgpu_decode_keyed_minmax_many_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                        const float* d_keys, uint32_t n_keys, alpgpu_zone_f32* d_out, uint64_t* d_counts);
int alpgpu_debug_decode_keyed_minmax_many_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                              const double* d_keys, uint32_t n_keys, alpgpu_zone_f64* d_out, uint64_t* d_counts, const alpgpu_keyed_tuning* tuning,
                                              uint64_t* d_trace);
int alpgpu_debug_decode_keyed_minmax_many_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                              const float* d_keys, uint32_t n_keys, alpgpu_zone_f32* d_out, uint64_t* d_counts, const alpgpu_keyed_tuning* tuning,
                                              uint64_t* d_trace);

/* ---- exact keyed SUM --------------------------------------------------------------------------------------------------------------------------------
 * SELECT key, SUM(x), COUNT(*) ... WHERE ... GROUP BY key for up to 2^20 discrete keys known in advance, in ONE pass that decodes both columns in
 * registers, each sum the CORRECTLY ROUNDED real sum of its rows.  Built for double and float columns (the first keyed SUM a float column gets).
 * alpgpu_decode_keyed_sum_* stops at 1024 keys because its sums are floating-point sums in a documented order; an exact sum needs no order.
 *   alpgpu_decode_keyed_exact_sum_*   val, key (val == key allowed), d_mask, d_key_zones, d_keys and n_keys (1 .. ALPGPU_KEYED_MANY_KEYS_MAX) are
 *                               alpgpu_decode_keyed_minmax_many_*'s, word for word, and so is the match: row r belongs to key i if i is the FIRST
 *                               position with d_keys[i] == k_r; -0.0 matches +0.0; a NaN k_r matches nothing and a NaN in d_keys is never matched;
 *                               later duplicates in d_keys receive nothing.  The zone-record rules are the same too: a record narrows its vector's
 *                               search; a record that admits no key means rows without a key, neither column read; min == max on a key vector
 *                               that is ALP without exceptions settles the key of every selected row without the key vector's packed words.
 *                               Truthful records change no byte.  Records that do not contain the truth, or keys that are not sorted, give
 *                               unspecified sums and counts; the sum of the n_keys + 1 counts is still the number of selected rows, and nothing
 *                               is read outside d_keys[0 .. n_keys) or the columns nor written outside the outputs and the table: every probe
 *                               index is clamped.
 *                               d_sums: n_keys doubles, 8-byte aligned, for both precisions (a float x_r is widened to double, exactly).
 *                               d_sums[i] is, over the selected rows of key i:
 *                                 a NaN (0x7FF8000000000000) if one of them is a NaN, or if +inf and -inf both occur;
 *                                 +inf / -inf if that infinity occurs;
 *                                 otherwise the real number sum of the x_r, rounded ONCE to the nearest double, ties to even: +-inf where that
 *                                 lies beyond DBL_MAX, exact where it is subnormal, +0.0 where it is zero (never -0.0, as in
 *                                 alpgpu_decode_keyed_sum_*; a key without rows and every later duplicate get +0.0).
 *                               There is no intermediate overflow and no cancellation error: DBL_MAX + DBL_MAX - DBL_MAX is DBL_MAX and
 *                               1e300 + 1 - 1e300 is 1.  The sums are a function of the inputs alone: the same bytes on every grid, device,
 *                               row order and sharding.
 *                               d_counts (may be NULL): n_keys + 1 words of 8 bytes, alpgpu_decode_keyed_minmax_many_*'s: d_counts[i] counts
 *                               every selected row of key i, the last word the selected rows without a key.  With NULL no count is kept.
 *                               d_table: alpgpu_keyed_exact_sum_table_bytes(n_keys) bytes of device memory owned by the caller, 16-byte aligned,
 *                               layout private (per key 66 limbs of int64, limb j of weight 2^(32 j - 1074), and a word of flags: NaN, +inf,
 *                               -inf seen).  Every value is added to its key's limbs as an integer, by integer atomics; the call ends with a
 *                               kernel that rounds every entry into d_sums.
 *                               accumulate == 0: a kernel zeroes the table and d_counts first (not a memset node: DESIGN.md, "Histograms").
 *                               accumulate != 0: the table is kept and added to, as alpgpu_histogram_*'s accumulate adds into its counts, and
 *                               d_counts, if given, is added to as well; d_sums is written from the table at the end of every call.  A second
 *                               call with accumulate on a shard of the columns, a range of a bitmap or another value column therefore extends
 *                               the sums exactly: partial tables add without error, and the result is that of one call over all the rows (the
 *                               same n_keys and keys; the table must come from a call with accumulate == 0 or be all zero bytes).
 *                               The bound.  A limb takes at most 2^32 - 1 per row, so it holds 2^31 rows.  One call refuses more than
 *                               ALPGPU_KEYED_EXACT_VECTORS_MAX = 2^21 vectors (2^31 rows); across accumulated calls the 2^31 rows per table are
 *                               the CALLER's bound: breaking it gives wrong sums and nothing else.
 *                               Cost: the zero kernel (536 bytes per key, the whole rounded up to 16), one launch of persistent workgroups sized to the device that stage
 *                               the keys as alpgpu_decode_keyed_minmax_many_* does, and the rounding kernel.  A step of 64 rows that agree on
 *                               their key and lie within 2^64 of each other is summed in registers and costs at most 5 integer atomics and one
 *                               for the count; any other row costs up to 3 integer atomics and one for its count.  No floating-point atomics,
 *                               no compare-and-swap loop, no workgroup waits for another.
 *                               n_vectors == 0: neither column is read; the table is zeroed (accumulate == 0) or kept and d_sums written from it.
 *                               ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx, val, key, d_keys, d_sums or d_table; n_keys outside
 *                               1 .. ALPGPU_KEYED_MANY_KEYS_MAX; columns that differ in n_vectors; n_vectors > ALPGPU_KEYED_EXACT_VECTORS_MAX;
 *                               d_sums, d_counts, d_mask or d_trace not 8-byte aligned; d_table not 16-byte aligned; d_key_zones not aligned to
 *                               its records, d_keys not aligned to its elements; with n_vectors > 0, a column without descriptors.
 *   alpgpu_keyed_exact_sum_table_bytes   536 * n_keys rounded up to a multiple of 16 (544 for one key), monotone; UINT64_MAX for n_keys outside 1 .. ALPGPU_KEYED_MANY_KEYS_MAX; host only.
 * The call runs on the context's stream and on that stream only: asynchronous, no host synchronisation, no allocation, no state kept; none of what
 *   the context remembers about columns is read or written; safe inside a stream capture (the keys, the bitmap and the table are read at replay).
 * The debug entry takes alpgpu_keyed_tuning (grid) and adds to SIX trace words: the four of alpgpu_debug_decode_keyed_sum_*, then
 *   [4] the steps of 64 rows summed in registers, [5] the steps sent to the table lane by lane.  No tuning changes a byte.
 * The name is keyed_exact_sum and not keyed_sum_exact: the entry points whose names hold "keyed_sum" are alpgpu_decode_keyed_sum_*'s family, the striped
 *   order, and are counted as such (tests/test_capi_refusals_cpu.py); the Python and C++ wrappers are keyed_sum_exact / sum_by_key_exact.
 * Not built: a table in LDS for few keys (up to 1024 keys alpgpu_decode_keyed_sum_f64 keeps its tables there), more than 2^20 keys per call,
 *   multi-column keys, keys not known in advance (alpgpu_distinct_* first).
 * TRUST: as for alpgpu_select_range_*. */
#define ALPGPU_KEYED_EXACT_VECTORS_MAX (1u << 21)
uint64_t alpgpu_keyed_exact_sum_table_bytes(uint32_t n_keys);
int alpgpu_decode_keyed_exact_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                      const double* d_keys, uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_table, int accumulate);
int alpgpu_decode_keyed_exact_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                      const float* d_keys, uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_table, int accumulate);
int alpgpu_debug_decode_keyed_exact_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                            const double* d_keys, uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_table, int accumulate,
                                            const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);
int alpgpu_debug_decode_keyed_exact_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                            const float* d_keys, uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_table, int accumulate,
                                            const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);

/* ---- bucketed aggregation -------------------------------------------------------------------------------------------------------------------------
 * SELECT width_bucket(key, edges), SUM(x) / MIN(x) / MAX(x), COUNT(*) ... WHERE ... GROUP BY 1: resampling a column into bins of a second column
 * (date_trunc(ts), OHLC bars, equi-width and equi-depth profiles), for up to 1024 buckets given by sorted edges, in ONE pass that decodes both
 * columns in registers, no decoded value reaching HBM.  The bucket is alpgpu_histogram_*'s, the tables are the keyed calls'.  Built for double and
 * float columns.
 *   alpgpu_decode_bucket_sum_* / alpgpu_decode_bucket_minmax_*
 *                               Rows.  val and key: two columns of the entry point's type with equal n_vectors; val == key is allowed.  Take every
 *                               row r whose bit is set in the bitmap (d_mask == NULL: every row).  x_r and k_r are, bit for bit, what
 *                               alpgpu_decode_* writes at r for val and for key, exceptions patched in; a float x_r is widened to double,
 *                               exactly, for the sums.
 *                               The bucket is alpgpu_histogram_*'s, word for word.  k_r a NaN (by the bits): the row is counted in
 *                               d_counts[n_edges + 1] and enters no sum and no record.  right == 0: b = #{i : d_edges[i] <= k_r}, the half-open
 *                               buckets [e[b-1], e[b]); right != 0: b = #{i : d_edges[i] < k_r}, the buckets (e[b-1], e[b]].  Bucket 0 lies
 *                               below the first edge and bucket n_edges at or above the last.  The comparisons are C's: -0.0 == +0.0, +-inf are
 *                               ordinary values and edges.  NaN edges, sorted last, are inert; duplicate edges give empty buckets.  n_edges == 0
 *                               is valid and d_edges may then be NULL: there is one bucket.  n_edges is at most ALPGPU_BUCKET_EDGES_MAX: the
 *                               n_edges + 1 buckets are the keyed calls' table entries.  d_edges: n_edges elements of the columns' type in
 *                               DEVICE memory, aligned to the element, sorted as numpy.sort sorts, read when the kernel runs (a captured graph
 *                               sees the edges' contents at replay; n_edges, right and the pointers are fixed at capture).
 *                               d_counts (may be NULL): n_edges + 2 words of 8 bytes, exact: the n_edges + 1 buckets' selected rows (NaN values
 *                               included) and, last, the rows whose key is a NaN.  They are, byte for byte, what alpgpu_histogram_* writes for
 *                               key over the whole column under the same bitmap, edges and right.  With d_counts == NULL
 *                               alpgpu_decode_bucket_minmax_* keeps no count at all.
 *                               d_sums (SUM): n_edges + 1 doubles in alpgpu_decode_keyed_sum_*'s order and no other, "belongs to key i" read as
 *                               "lies in bucket b": L = alpgpu_keyed_stripe_vectors(n_vectors); P(b, v, m) is the adjacent-lane tree over a
 *                               step's 64 lanes with +0.0 where a row is not selected or is not of bucket b; a stripe's partial starts at +0.0
 *                               and takes the steps in (v, m) order; alpgpu_tree_sum_f64 runs over the S stripes.  A selected NaN in val makes
 *                               its bucket's sum a NaN of unspecified payload.  Neither the grid, nor the device's CU count, nor the order in
 *                               which wavefronts arrive enters a bit.  A consequence: if d_edges are distinct keys without NaNs, right == 0 and
 *                               every selected key value is one of them or lies below the first, d_sums[i + 1] is, bit for bit,
 *                               alpgpu_decode_keyed_sum_f64's d_sums[i] for d_keys = d_edges, and d_sums[0] covers the rows below.
 *                               d_out (MIN / MAX): n_edges + 1 records {min, max} of the columns' type, aligned to the record (16 / 8 bytes), in
 *                               alpgpu_decode_minmax_masked_*'s order: NaN values ignored but counted, -0.0 < +0.0, a bucket without a number
 *                               gets {+inf, -inf}.  Exact and order-free: a function of the inputs alone.  Under the premise above record i + 1
 *                               is, byte for byte, alpgpu_decode_keyed_minmax_*'s record i.
 *                               d_mask (may be NULL): a selection bitmap of n_vectors * 16 words, 8-byte aligned, read and never written.  A vector
 *                               whose 16 words are zero costs its 128 bytes and nothing of either column.
 *                               d_key_zones (may be NULL; aligned to its records): any records that CONTAIN the true intervals of the KEY
 *                               vectors' selected values.  The rules are alpgpu_histogram_*'s, not the keyed calls': a record without a NaN
 *                               bound and with bucket(min) <= bucket(max) narrows the per-value search to the edges between the two.  If both
 *                               bounds lie in ONE bucket and the key vector's descriptor says ALP without exceptions, every selected row has
 *                               that bucket: the key vector's packed words are not requested and only the value vector is decoded.  This takes
 *                               min == max no longer: a sorted timestamp column with bins wider than a vector takes this route almost
 *                               everywhere.  A record with a NaN bound prunes nothing.  Truthful records change no byte.  Records that do not
 *                               contain the truth, or edges that are not sorted, give unspecified sums, records and per-bucket counts; the
 *                               n_edges + 2 counts still add up to the number of selected rows, nothing is read outside d_edges[0 .. n_edges) or
 *                               the columns and nothing is written outside the outputs: every probe index and every table index is clamped.
 *                               d_scratch (SUM): alpgpu_bucket_sum_scratch_bytes(n_vectors, n_edges) bytes, 16-byte aligned, contents irrelevant
 *                               before and unspecified after (alpgpu_decode_keyed_sum_*'s: the stripe ticket and S rows of n_edges + 1 doubles).
 *                               Cost: alpgpu_decode_keyed_sum_*'s (init kernel, persistent workgroups with private per-wavefront tables in two
 *                               capacity tiers, up to 256 and up to 1024 buckets, a reduce of one small workgroup per bucket) and
 *                               alpgpu_decode_keyed_minmax_*'s (init kernel, persistent workgroups with one table each on LDS integer atomics,
 *                               joined by global integer atomics); the edges take the keys' place in LDS.  A value costs
 *                               ceil(log2(n_edges + 1)) LDS probes, fewer under a zone record.
 *                               n_vectors == 0: +0.0, {+inf, -inf} and 0 everywhere, written by a kernel; neither column is read.
 *                               ALPGPU_ERR_INVALID before anything is enqueued: a NULL ctx, val, key, d_sums / d_out or d_scratch; a NULL d_edges
 *                               with n_edges > 0; n_edges > ALPGPU_BUCKET_EDGES_MAX; columns that differ in n_vectors; n_vectors > 2^32 - 1;
 *                               d_scratch not 16-byte aligned; d_sums, d_counts, d_mask or d_trace not 8-byte aligned; d_edges not aligned to its
 *                               elements, d_out or d_key_zones not aligned to their records; with n_vectors > 0, a column without descriptors.
 *   alpgpu_bucket_sum_scratch_bytes   alpgpu_keyed_sum_scratch_bytes(n_vectors, n_edges + 1); UINT64_MAX for n_edges > ALPGPU_BUCKET_EDGES_MAX.
 * The calls run on the context's stream and on that stream only: asynchronous, no host synchronisation, no allocation, no state kept; none of what
 *   the context remembers about columns is read or written; safe inside a stream capture (the edges and the bitmap are read at replay).  No
 *   floating-point atomics and no compare-and-swap loop; no workgroup waits for another.
 * The debug entries take alpgpu_keyed_tuning (grid) and add to four trace words, each wavefront once per word at its end.  They count vectors:
 *   [0] settled without either column (their bitmap words are all zero),
 *   [1] settled by the one-bucket shortcut (the key vector's packed words not requested),
 *   [2] always 0: every key that is not a NaN has a bucket,
 *   [3] decoded, both columns.
 *   No tuning changes a byte.
 * Not built: more than 1024 buckets per call (the reason alpgpu_decode_keyed_sum_* stops there: the tables sit in LDS), first / n sub-ranges,
 *   accumulate, multi-column keys, alpgpu_decode_keyed_sum_f32.
 * TRUST: as for alpgpu_select_range_*. */
#define ALPGPU_BUCKET_EDGES_MAX 1023u /* n_edges + 1 buckets <= ALPGPU_KEYED_KEYS_MAX table entries */
uint64_t alpgpu_bucket_sum_scratch_bytes(uint64_t n_vectors, uint32_t n_edges);
int alpgpu_decode_bucket_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                 const double* d_edges, uint32_t n_edges, int right, double* d_sums, uint64_t* d_counts, void* d_scratch);
int alpgpu_decode_bucket_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                 const float* d_edges, uint32_t n_edges, int right, double* d_sums, uint64_t* d_counts, void* d_scratch);
int alpgpu_decode_bucket_minmax_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                    const double* d_edges, uint32_t n_edges, int right, alpgpu_zone_f64* d_out, uint64_t* d_counts);
int alpgpu_decode_bucket_minmax_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                    const float* d_edges, uint32_t n_edges, int right, alpgpu_zone_f32* d_out, uint64_t* d_counts);
int alpgpu_debug_decode_bucket_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                       const double* d_edges, uint32_t n_edges, int right, double* d_sums, uint64_t* d_counts, void* d_scratch,
                                       const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);
int alpgpu_debug_decode_bucket_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                       const float* d_edges, uint32_t n_edges, int right, double* d_sums, uint64_t* d_counts, void* d_scratch,
                                       const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);
int alpgpu_debug_decode_bucket_minmax_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                          const double* d_edges, uint32_t n_edges, int right, alpgpu_zone_f64* d_out, uint64_t* d_counts,
                                          const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);
int alpgpu_debug_decode_bucket_minmax_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                          const float* d_edges, uint32_t n_edges, int right, alpgpu_zone_f32* d_out, uint64_t* d_counts,
                                          const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);

/* Opt-in guard for device-resident columns of unknown origin: one pass over the descriptors on the device checks, for every vector,
 * scheme (and that it is its rowgroup's), widths, exponent / factor, exception count, alignment, that its packed words and its
 * exception record lie inside packed_capacity / exc_capacity, and that every exception position is < 1024.  value_bytes = 8
 * (double column) or 4 (float column).  Synchronises the stream; ALPGPU_OK, or ALPGPU_ERR_INVALID with *first_bad = the lowest
 * offending vector index (optional). */
int alpgpu_column_validate(alpgpu_ctx* ctx, const alpgpu_column* col, int value_bytes, uint64_t* first_bad);

/* host copy of d_totals after the stream has drained: packed bytes, exception bytes, overflow flag */
int alpgpu_column_totals(alpgpu_ctx* ctx, alpgpu_column* col, uint64_t* packed_bytes, uint64_t* exc_bytes, int* overflow);

/* ---- tail padding and a serialized container ---------------------------------------------
 * The codec works on whole 1024-value vectors (reference PRIMITIVES.md:141-144 leaves incomplete last vectors to the
 * caller; its drivers drop them).  alpgpu_pad_tail_f64 fills d_in[n_values .. next multiple of 1024) with the first
 * value of the incomplete vector; d_in must have room for that many doubles.  Encode ceil(n_values/1024) vectors. */
int alpgpu_pad_tail_f64(alpgpu_ctx* ctx, double* d_in, uint64_t n_values);

/* Blob = 64-byte header, rowgroup states, vector descriptors, packed stream, exception stream (all little-endian,
 * exactly the HBM records of this header).  Host memory.  Both calls synchronise the context's stream. */
typedef struct alpgpu_blob_header {
	char     magic[8];      /* "ALPGPU1\0" */
	uint32_t version;       /* 1 */
	uint32_t header_bytes;  /* 64 */
	uint64_t n_values;      /* values that are data (<= n_vectors * 1024; the rest is tail padding) */
	uint64_t n_vectors;
	uint64_t n_rowgroups;
	uint64_t packed_bytes;
	uint64_t exc_bytes;
	uint64_t reserved;       /* value type: 0 or 8 = double column, 4 = float column */
} alpgpu_blob_header;
uint64_t alpgpu_blob_size(uint64_t n_vectors, uint64_t packed_bytes, uint64_t exc_bytes);
int      alpgpu_column_to_blob(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t n_values, void* h_blob, uint64_t capacity,
                               uint64_t* written);
/* validates the blob and copies it into the caller-allocated column buffers.  Nothing is copied, and no kernel runs, before the whole blob has passed.
 * The header must satisfy, in this order (ALPGPU_ERR_INVALID otherwise):
 *   size >= 64;  magic "ALPGPU1\0", version 1, header_bytes 64;  reserved names the entry point's value type (0 or 8: double, 4: float);
 *   n_rowgroups == ceil(n_vectors / 100);  n_values lies in the last vector: (n_vectors - 1) * 1024 < n_values <= n_vectors * 1024, and 0 for no vectors;
 *   packed_bytes <= 2^56 and exc_bytes <= 2^56;
 *   64 + 32 * n_rowgroups + 32 * n_vectors + packed_bytes rounded up to 8 + exc_bytes rounded up to 8 <= size (bytes behind that are ignored).
 * These are statements about integers: the validator evaluates them so that no field value can make one of its expressions wrap (n_vectors is bounded
 * by size / 32 before anything is multiplied), so no field value can make it read outside [h_blob, h_blob + size).
 * Then every descriptor, in vector order; the first that fails ends the call:
 *   scheme is ALP or ALP_RD and equals its rowgroup's;
 *   ALP: bw <= 64 (float: 32), e <= 18 (float: 10), f <= e.  ALP_RD: bw <= 63 (float: 31), 1 <= lbw <= 3, bw and lbw equal the rowgroup's rd_rbw and
 *   rd_lbw.  exc_cnt <= 1024.  Fields documented as unused for the scheme (an ALP vector's lbw; an ALP_RD vector's e, f and base) may hold anything:
 *   no kernel reads them for that scheme;
 *   packed_off is a multiple of 128, exc_off of 8, and both records lie inside their streams: packed_off + 128 * bw (ALP_RD: + 128 * lbw) <= packed_bytes,
 *   exc_off + the record's size (exc_cnt values of 8 / 4 bytes, ALP_RD: 2 bytes, then exc_cnt 2-byte positions, rounded up to 8) <= exc_bytes.  A record
 *   of no bytes may sit at the stream's end.  Records may overlap and lie in any order here (alpgpu_decompress_host_* also wants every record inside
 *   its chunk's stream range, which offsets that ascend with the vector index give);
 *   every exception position is < 1024.
 * The same rules, from the same function, are what alpgpu_column_validate holds a device column to (alp_amd/csrc/blob_check.hpp). */
int      alpgpu_column_from_blob(alpgpu_ctx* ctx, const void* h_blob, uint64_t size, alpgpu_column* col, uint64_t* n_values);

/* ---- vector primitives on batches (fixed strides; the reference's per-vector API, n at a time) ------
 * Each processes n_vectors independent vectors.  "stride" arguments are in ELEMENTS of the pointed type
 * between consecutive vectors (the reference's callers use 1024-element buffers for everything).
 * What tests/test_primitive_batches_gpu.py pins beyond that:
 *   - every packed row (d_packed + v * packed_stride) must be 16-byte aligned: the 64- and 32-bit lanes move packed words 16 bytes at a
 *     time.  A 16-byte aligned d_packed and any stride that is a multiple of the tight one (16 / 32 / 64 / 128 elements per bit of the
 *     batch's largest width for 64 / 32 / 16 / 8-bit lanes) satisfy it.  A vector touches only the first 128 * bw bytes of its row.
 *   - a width above the lane width (bw > 64 / 32 / 16 / 8) is a no-op, as in the reference's switch: ffor, unffor and falp leave that
 *     vector's output untouched.  bw = 0: ffor writes nothing, unffor gives the base.
 *   - exception rows: only the first cnt entries of a vector's d_exc / d_pos row are written (encoders) or read (patch, rd_decode);
 *     exc_stride must be at least the batch's largest count.
 *   - rd_encode_vectors_* writes dict_size as the left index of an exception; rd_decode_vectors_* accepts any index there (an index
 *     of 8 or more reads no dictionary entry), the exception list overwrites the slot. */

/* ffor::ffor / unffor::unffor, 64-bit lanes: in/out [n][1024] int64, packed [n][packed_stride] (>= 16*bw words
 * used per vector), bw/base per vector */
int alpgpu_ffor_i64(alpgpu_ctx* ctx, const int64_t* d_in, int64_t* d_packed, size_t packed_stride,
                    const uint8_t* d_bw, const int64_t* d_base, uint64_t n_vectors);
int alpgpu_unffor_i64(alpgpu_ctx* ctx, const int64_t* d_packed, size_t packed_stride, int64_t* d_out,
                      const uint8_t* d_bw, const int64_t* d_base, uint64_t n_vectors);
/* 16-bit lanes (ALP_RD left parts) */
int alpgpu_ffor_u16(alpgpu_ctx* ctx, const uint16_t* d_in, uint16_t* d_packed, size_t packed_stride,
                    const uint8_t* d_bw, const uint16_t* d_base, uint64_t n_vectors);
int alpgpu_unffor_u16(alpgpu_ctx* ctx, const uint16_t* d_packed, size_t packed_stride, uint16_t* d_out,
                      const uint8_t* d_bw, const uint16_t* d_base, uint64_t n_vectors);

/* 8-bit lanes (128 lane-streams x 8 rows; not used by the codec, part of the reference's ffor/unffor API: include/fastlanes/ffor.hpp:10) */
int alpgpu_ffor_u8(alpgpu_ctx* ctx, const uint8_t* d_in, uint8_t* d_packed, size_t packed_stride, const uint8_t* d_bw,
                   const uint8_t* d_base, uint64_t n_vectors);
int alpgpu_unffor_u8(alpgpu_ctx* ctx, const uint8_t* d_packed, size_t packed_stride, uint8_t* d_out, const uint8_t* d_bw,
                     const uint8_t* d_base, uint64_t n_vectors);

/* falp without exception patching: packed -> doubles */
int alpgpu_falp_f64(alpgpu_ctx* ctx, const int64_t* d_packed, size_t packed_stride, double* d_out,
                    const uint8_t* d_bw, const int64_t* d_base, const uint8_t* d_fac, const uint8_t* d_exp,
                    uint64_t n_vectors);
/* decoder::decode: encoded integers -> doubles */
int alpgpu_decode_values_f64(alpgpu_ctx* ctx, const int64_t* d_enc, double* d_out, const uint8_t* d_fac,
                             const uint8_t* d_exp, uint64_t n_vectors);
/* decoder::patch_exceptions: out[pos[j]] = exc[j]; exc/pos [n][exc_stride] */
int alpgpu_patch_f64(alpgpu_ctx* ctx, double* d_out, const double* d_exc, const uint16_t* d_pos, size_t exc_stride,
                     const uint16_t* d_cnt, uint64_t n_vectors);
/* encoder::encode_simdized with a given (fac, exp) per vector: -> enc [n][1024], exc/pos [n][exc_stride], cnt [n] */
int alpgpu_encode_simdized_f64(alpgpu_ctx* ctx, const double* d_in, double* d_exc, uint16_t* d_pos, size_t exc_stride,
                               uint16_t* d_cnt, int64_t* d_enc, const uint8_t* d_fac, const uint8_t* d_exp,
                               uint64_t n_vectors);
/* encoder::encode (second-level sampling when state.k > 1, then encode_simdized); one state per vector
 * (d_state_idx[v] indexes d_states; NULL = vector v uses state v/100); chosen (fac, exp) are returned */
int alpgpu_encode_values_f64(alpgpu_ctx* ctx, const double* d_in, const alpgpu_rowgroup_state* d_states,
                             const uint32_t* d_state_idx, double* d_exc, uint16_t* d_pos, size_t exc_stride,
                             uint16_t* d_cnt, int64_t* d_enc, uint8_t* d_fac, uint8_t* d_exp, uint64_t n_vectors);
/* encoder::encode_value<SAFE> (include/alp/encoder.hpp:81-89), the scalar helper of the reference's header, on n_values VALUES (not vectors)
 * with ONE (factor, exponent) pair: d_enc[i] = the encoded integer of d_in[i]; safe != 0 gives the sampling form (the sentinel
 * ENCODING_UPPER_LIMIT for values that cannot be encoded), 0 the plain one (x86 cast semantics).  _f32: `safe` is ignored, the float SAFE
 * branch does not exist in the reference as built. */
int alpgpu_encode_value_f64(alpgpu_ctx* ctx, const double* d_in, int64_t* d_enc, uint8_t fac, uint8_t exp, int safe, uint64_t n_values);
int alpgpu_encode_value_f32(alpgpu_ctx* ctx, const float* d_in, int32_t* d_enc, uint8_t fac, uint8_t exp, int safe, uint64_t n_values);
/* encoder::analyze_ffor */
int alpgpu_analyze_ffor_i64(alpgpu_ctx* ctx, const int64_t* d_enc, uint8_t* d_bw, int64_t* d_base, uint64_t n_vectors);

/* rd_encoder::encode / decode with per-vector state index as above */
int alpgpu_rd_encode_vectors_f64(alpgpu_ctx* ctx, const double* d_in, const alpgpu_rowgroup_state* d_states,
                                 const uint32_t* d_state_idx, uint16_t* d_exc, uint16_t* d_pos, size_t exc_stride,
                                 uint16_t* d_cnt, uint64_t* d_right, uint16_t* d_left, uint64_t n_vectors);
int alpgpu_rd_decode_vectors_f64(alpgpu_ctx* ctx, double* d_out, const uint64_t* d_right, const uint16_t* d_left,
                                 const alpgpu_rowgroup_state* d_states, const uint32_t* d_state_idx,
                                 const uint16_t* d_exc, const uint16_t* d_pos, size_t exc_stride,
                                 const uint16_t* d_cnt, uint64_t n_vectors);
/* the same two under the names SURVEY.md §8(b) lists (alpgpu_rd_encode_f64 / alpgpu_rd_decode_f64) */
int alpgpu_rd_encode_f64(alpgpu_ctx* ctx, const double* d_in, const alpgpu_rowgroup_state* d_states, const uint32_t* d_state_idx,
                         uint16_t* d_exc, uint16_t* d_pos, size_t exc_stride, uint16_t* d_cnt, uint64_t* d_right, uint16_t* d_left,
                         uint64_t n_vectors);
int alpgpu_rd_decode_f64(alpgpu_ctx* ctx, double* d_out, const uint64_t* d_right, const uint16_t* d_left,
                         const alpgpu_rowgroup_state* d_states, const uint32_t* d_state_idx, const uint16_t* d_exc,
                         const uint16_t* d_pos, size_t exc_stride, const uint16_t* d_cnt, uint64_t n_vectors);

/* ==== single precision ====================================================================
 * The float instantiation of the same API: alp::encoder<float> / decoder<float> / rd_encoder<float> (same files and
 * lines as the double entries above), Constants<float> include/alp/constants.hpp:30-64 (66 (e,f) candidates, exception
 * cost 32+16 bits, ALP_RD threshold 22*32), falp float include/alp/falp.hpp:28-44, 32-bit FFOR
 * src/fastlanes_generated_ffor.cpp:1776-7378 (32 lanes x 32 rows).  The column records are the same structs with
 *   packed stream : ALP 128*bw bytes (bw 0..32); ALP_RD 128*rbw (right, u32 lanes, rbw 16..31) then 128*lbw (left, u16 lanes)
 *   exception rec.: ALP cnt*4 B values (f32 bits) then cnt*2 B positions; ALP_RD cnt*2 B left parts then cnt*2 B positions;
 *                   rounded up to 8 bytes
 *   vector_desc.base: the int32 frame-of-reference base, sign-extended.
 * A column encoded by the _f32 functions must be decoded by alpgpu_decode_f32 (the records do not carry the value type;
 * blobs do: alpgpu_blob_header.reserved = 4 for float columns).
 * Behaviour where the reference's float code is undefined in C++ (out-of-range float->int32 casts, the SAFE branch of
 * encode_value, FACT_ARR[10]) follows the reference AS BUILT with Clang, pinned by oracle/alp_oracle_f32.c (see its header). */
uint64_t alpgpu_packed_capacity_f32(uint64_t n_vectors); /* worst case n_vectors * 4352 */
uint64_t alpgpu_exc_capacity_f32(uint64_t n_vectors);    /* worst case n_vectors * 6144 */
int alpgpu_rowgroup_init_f32(alpgpu_ctx* ctx, const float* d_in, uint64_t n_vectors, alpgpu_column* col);
int alpgpu_state_from_samples_f32(alpgpu_ctx* ctx, const float* d_samples, uint32_t n_samples, alpgpu_rowgroup_state* d_state);
int alpgpu_rd_state_from_samples_f32(alpgpu_ctx* ctx, const float* d_samples, uint32_t n_samples, alpgpu_rowgroup_state* d_state);
int alpgpu_encode_vectors_f32(alpgpu_ctx* ctx, const float* d_in, uint64_t n_vectors, alpgpu_column* col);
int alpgpu_encode_f32(alpgpu_ctx* ctx, const float* d_in, uint64_t n_vectors, alpgpu_column* col);
/* ALPGPU_OPT_DECODE_VECTORS_PER_WG applies with values 0 (auto), 1, 2, 4 (float: four vectors over the full stage), 8 and 16..30 (see the option) */
int alpgpu_decode_f32(alpgpu_ctx* ctx, const alpgpu_column* col, float* d_out);
/* The fused consumers of alpgpu_decode_sum_f64 / alpgpu_decode_count_range_f64 for float columns.  Sums accumulate in double
 * (every float widens exactly): thread t = 64 w + L of 256 adds values 4t, 4t+1, 4t+2, 4t+3 in that order starting from 0, giving
 * p[w][L]; then s[L] = (p[0][L] + p[1][L]) + (p[2][L] + p[3][L]); then the balanced tree over adjacent lanes over the 64 s[L] (as for
 * double; earlier in round 3 each wavefront ran the tree first).  ALPGPU_OPT_CONSUMER_PIPELINED: 0 / 2 = one wavefront per vector (the
 * default for float columns whatever they hold), 1 / 3 = the staged four-wavefront kernel; same bits.
 * Round 6: in an ALP vector the exception POSITIONS are skipped in the quads (they contribute nothing to p[w][L]) and the exception VALUES
 * join behind them, in the order of the record: s[L] += (double)exc[j] for j = L, L + 64, L + 128, ... before the tree.  ALP_RD vectors: as
 * before, every value in its place.  (tests/test_decode_sum_gpu.py: host_sums_f32 is the replica.) */
int alpgpu_decode_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_sums);
int alpgpu_decode_count_range_f32(alpgpu_ctx* ctx, const alpgpu_column* col, float lo, float hi, uint32_t* d_counts);
int alpgpu_pad_tail_f32(alpgpu_ctx* ctx, float* d_in, uint64_t n_values);
int alpgpu_column_to_blob_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t n_values, void* h_blob, uint64_t capacity, uint64_t* written);
int alpgpu_column_from_blob_f32(alpgpu_ctx* ctx, const void* h_blob, uint64_t size, alpgpu_column* col, uint64_t* n_values);
/* batch primitives, 32-bit lanes (same conventions as the 64-bit ones above) */
int alpgpu_ffor_i32(alpgpu_ctx* ctx, const int32_t* d_in, int32_t* d_packed, size_t packed_stride, const uint8_t* d_bw,
                    const int32_t* d_base, uint64_t n_vectors);
int alpgpu_unffor_i32(alpgpu_ctx* ctx, const int32_t* d_packed, size_t packed_stride, int32_t* d_out, const uint8_t* d_bw,
                      const int32_t* d_base, uint64_t n_vectors);
int alpgpu_falp_f32(alpgpu_ctx* ctx, const int32_t* d_packed, size_t packed_stride, float* d_out, const uint8_t* d_bw,
                    const int32_t* d_base, const uint8_t* d_fac, const uint8_t* d_exp, uint64_t n_vectors);
int alpgpu_decode_values_f32(alpgpu_ctx* ctx, const int32_t* d_enc, float* d_out, const uint8_t* d_fac, const uint8_t* d_exp,
                             uint64_t n_vectors);
int alpgpu_patch_f32(alpgpu_ctx* ctx, float* d_out, const float* d_exc, const uint16_t* d_pos, size_t exc_stride,
                     const uint16_t* d_cnt, uint64_t n_vectors);
int alpgpu_encode_simdized_f32(alpgpu_ctx* ctx, const float* d_in, float* d_exc, uint16_t* d_pos, size_t exc_stride, uint16_t* d_cnt,
                               int32_t* d_enc, const uint8_t* d_fac, const uint8_t* d_exp, uint64_t n_vectors);
int alpgpu_encode_values_f32(alpgpu_ctx* ctx, const float* d_in, const alpgpu_rowgroup_state* d_states, const uint32_t* d_state_idx,
                             float* d_exc, uint16_t* d_pos, size_t exc_stride, uint16_t* d_cnt, int32_t* d_enc, uint8_t* d_fac,
                             uint8_t* d_exp, uint64_t n_vectors);
int alpgpu_analyze_ffor_i32(alpgpu_ctx* ctx, const int32_t* d_enc, uint8_t* d_bw, int32_t* d_base, uint64_t n_vectors);
int alpgpu_rd_encode_vectors_f32(alpgpu_ctx* ctx, const float* d_in, const alpgpu_rowgroup_state* d_states, const uint32_t* d_state_idx,
                                 uint16_t* d_exc, uint16_t* d_pos, size_t exc_stride, uint16_t* d_cnt, uint32_t* d_right,
                                 uint16_t* d_left, uint64_t n_vectors);
int alpgpu_rd_decode_vectors_f32(alpgpu_ctx* ctx, float* d_out, const uint32_t* d_right, const uint16_t* d_left,
                                 const alpgpu_rowgroup_state* d_states, const uint32_t* d_state_idx, const uint16_t* d_exc,
                                 const uint16_t* d_pos, size_t exc_stride, const uint16_t* d_cnt, uint64_t n_vectors);

#ifdef __cplusplus
}
#endif
#endif /* ALPGPU_H */
