// host_ctx.hpp — what the translation units behind include/alpgpu.h share (internal to libalpgpu.so): the context, the error text, the argument-check
// macros and the few helpers more than one of them uses.  The extern "C" surface is spread over
//   api_context.hip    contexts, options, streams, memory, the scan workspace
//   api_encode.hip     rowgroup search + vector encode entry points (and the encode's measurement probes)
//   api_decode.hip     the store decode's entry points and the host state of its launch plan (segment tables, learn slots, streams and events), the fused
//                      consumers, alpgpu_column_totals; the launch RULE itself is decode_policy.hpp: pure functions, shared with the device and the CPU tests
//   api_primitives.hip the reference's per-vector primitives in batch form
//   api_container.hip  the serialized column (blob) and the descriptor checks
//   api_host.hip       columns that live in host memory: the chunked two-stream pipelines, one or several contexts
// No codec arithmetic lives in any of them and there is no CPU path: without a gfx950 device alpgpu_ctx_create fails and nothing else can be called.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/alpgpu.h"
#include "launch.hpp"

#define ALPGPU_INTERNAL __attribute__((visibility("hidden")))

// Per-segment sizes of a column (segments of seg_vectors consecutive vectors, a multiple of 400): what a launch rule that sees more than the column's
// averages needs.  Host-side, in the context, keyed by the descriptor buffer: struct alpgpu_column stays as it is (ABI 3).
constexpr int kMaxSegments = 32;
struct SegmentTable {
	const void* key;         // col->d_vectors (nullptr: empty slot)
	const void* d_packed;    // ... and the rest of what a column must share with the one the sums were taken from: a caching allocator hands the same
	uint64_t    n_vectors;   //     descriptor buffer to the next column of the same length, whose stream sizes then differ
	uint64_t    packed_bytes, exc_bytes;
	uint64_t    seg_vectors;
	uint32_t    n_seg;
	uint64_t    packed[kMaxSegments];  // bytes of packed records
	uint64_t    exc_cnt[kMaxSegments]; // exceptions
	uint64_t    rd_vectors[kMaxSegments]; // vectors of ALP_RD rowgroups
};

// What an UNHINTED decode learned about a column (api_decode.hip: decode_unhinted): the per-segment sums taken on the stream travel to page-locked host words behind
// an event that is only ever queried; once there, the next decode of the same column is planned on the host.  state 0: empty, 1: copy in flight, 2: sizes known,
// 3: abandoned with its copy perhaps still in flight (the column was encoded again: segment_table_forget) — reused once its event has completed, never waited for.
// A decode enqueued on a capturing stream neither reads nor writes slots: an event recorded and a copy made only in a graph would land at some later replay.
constexpr int kLearnSlots = 4;
struct LearnSlot {
	const void* key;       // col->d_vectors
	const void* d_packed;
	uint64_t    n_vectors;
	int         value_bytes;
	uint32_t    n_seg;
	int         state;
	hipEvent_t  ev;
	uint64_t    packed, exceptions, rd_vectors;
};

struct alpgpu_ctx {
	int         device;
	hipStream_t own_stream;
	hipStream_t stream;
	int         n_cus;
	alpgpu::DecodeOptions decode_opt; // what the store decode's launch rule takes from alpgpu_set_option (decode_policy.hpp): forced shape, forced pad, read-ahead, plain stores
	char        name[128];
	uint64_t    hbm_bytes;
	int         encode_two_pass; // 0 (default): single-pass encode with look-back offsets; 1: analysis + scan + pack
	int         force_stall;     // debug: the single pass gives up in its look-back, the recovery route re-encodes
	int         async_init;      // 1 (default): alpgpu_encode_* of a long column runs the rowgroup search BESIDE the vector encode (second stream)
	hipStream_t init_stream;     // ... on this stream (highest priority: its few workgroups are placed first)
	hipEvent_t  ev_fork, ev_head, ev_join;
	int         encode_unordered; // ALPGPU_OPT_ENCODE_UNORDERED: tiles reserve their stream bytes with one atomic add (lean kernel, device columns only)
	int         read_ahead_us;     // the read-ahead (decode_opt.read_ahead; read_ahead_kernels.hip) runs this many microseconds ahead of the decode kernel (0: 12 + 6.5 us per packed bit of the vectors, at most 60)
	uint64_t*   d_progress;        // ... paced by this word of device memory (2 KiB; the map of its words: decode_policy.hpp)
	uint64_t    progress_gen;      // ... whose tag changes with every launch
	uint32_t    wall_tick_ps;      // picoseconds per tick of the device's wall_clock64() (the read-ahead's naps)
	int         decode_segments;   // ALPGPU_OPT_DECODE_SEGMENTS: a column whose regions differ is decoded region by region, each with its own launch shape (1, default)
	SegmentTable seg_tables[4];    // ... from the per-segment sizes alpgpu_column_totals / alpgpu_column_from_blob last saw (host-side, keyed by the descriptor buffer)
	int         seg_next;
	int         decode_unhinted;   // ALPGPU_OPT_DECODE_UNHINTED (1, default): a column whose sizes the host does not know gets them summed on the stream and its launch shape chosen on the device
	LearnSlot   learn[kLearnSlots]; // ... and what those sums said, for the next decode of the same column
	int         learn_next;
	uint64_t*   h_learn;           // page-locked: kLearnSlots x 3 x kMaxSegments words
	int         pipelined_consumer; // 1: the fused consumers through the persistent LDS-ring kernel (consume_kernels.hip; its own summation order)
	void*       workspace;       // scan workspace (tile sums / tile status words), grown on demand
	uint64_t    workspace_bytes;
	hipEvent_t  ws_event;        // recorded behind the last encode that used the workspace ...
	hipStream_t ws_stream;       // ... on this stream
	int         ws_busy;
};

namespace alpgpu_host {
extern thread_local char g_err[512];
ALPGPU_INTERNAL int fail(int code, const char* what, hipError_t e = hipSuccess);
} // namespace alpgpu_host
using alpgpu_host::fail;
using alpgpu_host::g_err;

#define ALPGPU_HIP(call)                                                                                                \
	do {                                                                                                                \
		hipError_t e_ = (call);                                                                                         \
		if (e_ != hipSuccess) { return fail(ALPGPU_ERR_HIP, #call, e_); }                                               \
	} while (0)

#define ALPGPU_CHECK_CTX(ctx)                                                                                           \
	do {                                                                                                                \
		if (!(ctx)) { return fail(ALPGPU_ERR_INVALID, "null context"); }                                                \
		ALPGPU_HIP(hipSetDevice((ctx)->device));                                                                        \
	} while (0)

// an argument check (below) or a helper that has already called fail(): its error is the entry point's
#define ALPGPU_TRY(call)                                                                                                \
	do {                                                                                                                \
		const int rc_ = (call);                                                                                         \
		if (rc_ != ALPGPU_OK) { return rc_; }                                                                           \
	} while (0)

#define ALPGPU_PRIM(cond_ok, call)                                                                                      \
	do {                                                                                                                \
		ALPGPU_CHECK_CTX(ctx);                                                                                          \
		if (n_vectors && !(cond_ok)) { return fail(ALPGPU_ERR_INVALID, "null pointer argument"); }                      \
		if ((call) != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "kernel launch failed", hipGetLastError()); }            \
		return ALPGPU_OK;                                                                                               \
	} while (0)

// ---- helpers shared between the translation units (hidden: not part of the ABI) ----
extern "C" {
// api_context.hip: one scan / status workspace per context, ordered behind its previous user
ALPGPU_INTERNAL int ensure_workspace(alpgpu_ctx* ctx, uint64_t bytes);
ALPGPU_INTERNAL int workspace_used(alpgpu_ctx* ctx);
ALPGPU_INTERNAL int check_column(const alpgpu_column* col, uint64_t n_vectors);
// api_decode.hip: the per-segment sizes the decode's launch plan is made from (a column that is encoded again has new regions)
constexpr uint64_t kSegmentMinVectors = 32800; // a multiple of 400: runs begin on rowgroup boundaries and on even vectors
ALPGPU_INTERNAL void          segment_table_forget(alpgpu_ctx* ctx, const alpgpu_column* col);
ALPGPU_INTERNAL uint64_t      segment_vectors_for(uint64_t n_vectors);
ALPGPU_INTERNAL SegmentTable* segment_table_new(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t packed_bytes, uint64_t exc_bytes);
// api_container.hip: a serialized column's header and descriptors, checked on the host
ALPGPU_INTERNAL int  validate_blob_header(const void* h_blob, uint64_t size, uint64_t value_bytes, alpgpu_blob_header& h);
ALPGPU_INTERNAL int  validate_blob_vectors(const void* h_blob, const alpgpu_blob_header& h, uint64_t value_bytes, uint64_t v_begin, uint64_t v_end, const uint64_t* window = nullptr);
} // extern "C"
inline uint64_t align8(uint64_t x) { return (x + 7ull) & ~7ull; }
// p does not lie on a multiple of `bytes` (a power of two); a null pointer never is misaligned
inline bool misaligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) != 0; }

// ---- argument checks that several entry points make (api_mask, api_pair, api_in_list, api_select, api_group, api_minmax, api_top_k, api_quantile, api_zone): each
// returns ALPGPU_OK or fail(...); hidden, like the helpers above.  An entry point calls them in the order in which it reports its errors.
ALPGPU_INTERNAL inline int check_mask_op(int op) {
	if (op != ALPGPU_MASK_SET && op != ALPGPU_MASK_AND && op != ALPGPU_MASK_OR) { return fail(ALPGPU_ERR_INVALID, "op is none of ALPGPU_MASK_SET / _AND / _OR"); }
	return ALPGPU_OK;
}
// n_vectors << 10, the number of values, must not overflow; text: "column.n_vectors is implausible" or "n_vectors is implausible", as the caller knows it
ALPGPU_INTERNAL inline int check_n_vectors(uint64_t n_vectors, const char* text) {
	if (n_vectors > (~0ull >> 10)) { return fail(ALPGPU_ERR_INVALID, text); }
	return ALPGPU_OK;
}
// [first, first + n) lies within the n_vectors << 10 values (check_n_vectors came first); text: "range reaches past the column's last value" or "... columns' ..."
ALPGPU_INTERNAL inline int check_value_range(uint64_t n_vectors, uint64_t first, uint64_t n, const char* text) {
	const uint64_t n_values = n_vectors << 10;
	if (first > n_values || n > n_values - first) { return fail(ALPGPU_ERR_INVALID, text); } // (first + n without the overflow)
	return ALPGPU_OK;
}
ALPGPU_INTERNAL inline int check_bitmap_aligned(const void* d_mask) {
	if (misaligned(d_mask, 8u)) { return fail(ALPGPU_ERR_INVALID, "bitmap is not 8-byte aligned"); }
	return ALPGPU_OK;
}
ALPGPU_INTERNAL inline int check_has_descriptors(const alpgpu_column* col) {
	if (!col->d_vectors || !col->d_rowgroups) { return fail(ALPGPU_ERR_INVALID, "column has no descriptors"); }
	return ALPGPU_OK;
}
ALPGPU_INTERNAL inline int check_has_descriptors(const alpgpu_column* a, const alpgpu_column* b) {
	ALPGPU_TRY(check_has_descriptors(a));
	return check_has_descriptors(b);
}
// ---- what the keyed and bucketed aggregations (api_keyed, api_keyed_minmax, api_keyed_minmax_many, api_bucket) check alike; each entry point calls them
// in the order in which it has always reported its errors, between its own checks.  Null pointers are aligned.
// the two columns (non-null)
ALPGPU_INTERNAL inline int check_pair_n_vectors(const alpgpu_column* val, const alpgpu_column* key) {
	if (val->n_vectors != key->n_vectors) { return fail(ALPGPU_ERR_INVALID, "the columns differ in n_vectors"); }
	if (val->n_vectors > 0xFFFFFFFFull) { return fail(ALPGPU_ERR_INVALID, "column.n_vectors is beyond 2^32 - 1"); }
	return ALPGPU_OK;
}
ALPGPU_INTERNAL inline int check_bitmap_counts_trace(const uint64_t* d_mask, const uint64_t* d_counts, const uint64_t* d_trace) {
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	if (misaligned(d_counts, 8u) || misaligned(d_trace, 8u)) { return fail(ALPGPU_ERR_INVALID, "counts or trace are not 8-byte aligned"); }
	return ALPGPU_OK;
}
// the sorted list (list_text: "keys are not aligned to their elements" / "edges are ...") and the key column's zone records
ALPGPU_INTERNAL inline int check_list_and_zones(const void* d_list, const char* list_text, const void* d_zones, int value_bytes) {
	if (misaligned(d_list, static_cast<unsigned>(value_bytes))) { return fail(ALPGPU_ERR_INVALID, list_text); }
	if (misaligned(d_zones, 2u * value_bytes)) { return fail(ALPGPU_ERR_INVALID, "zones are not aligned to their records"); }
	return ALPGPU_OK;
}
// the last step of the three MIN / MAX calls: an empty column gets {+inf, -inf} in its n_records records and 0 in its n_records + 1 counts by a kernel
// and *done is set; otherwise the columns must have descriptors
ALPGPU_INTERNAL inline int minmax_empty_or_descriptors(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, void* d_out, uint64_t* d_counts, uint32_t n_records,
                                                       int value_bytes, bool* done) {
	*done = val->n_vectors == 0;
	if (*done) {
		if (alpgpu::launch_keyed_minmax_init(ctx->stream, d_out, d_counts, n_records, value_bytes) != ALPGPU_OK) {
			return fail(ALPGPU_ERR_HIP, "emptying the records and counts failed", hipGetLastError());
		}
		return ALPGPU_OK;
	}
	return check_has_descriptors(val, key);
}
// a bitmap entry point whose range is empty (n == 0): nothing qualifies, so SET and AND clear every bit and OR changes none
ALPGPU_INTERNAL inline int clear_bitmap_for_empty_range(alpgpu_ctx* ctx, int op, uint64_t* d_mask, const alpgpu_column* col) {
	if (op != ALPGPU_MASK_OR) { ALPGPU_HIP(hipMemsetAsync(d_mask, 0, 128ull * col->n_vectors, ctx->stream)); }
	return ALPGPU_OK;
}
