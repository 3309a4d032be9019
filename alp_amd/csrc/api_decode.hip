// api_decode.hip — the store decode's entry points and the HOST STATE its launch plan lives in (the per-segment tables of a column decoded region by region, what an unhinted
// decode learned, the streams and events of the read-ahead), the fused consumers and alpgpu_column_totals (which records what the plan needs) of include/alpgpu.h (see host_ctx.hpp for
// the map).  The launch RULE — shape, residency, read-ahead — is decode_policy.hpp: pure functions of a stretch's sizes and the context's options, evaluated once per launch (planned).
#include "decode_policy.hpp"
#include "host_ctx.hpp"

constexpr int      kReadAheadGrid    = 64;  // the read-ahead's eight-wavefront workgroups
constexpr uint32_t kReadAheadMaxBits = 128; // ... read the records of vectors of at most this many packed bits per value (the descriptors of all)

extern "C" {

// the launch of this column (or run) as a whole, from its size hints and the context's options
static alpgpu::DecodePlan planned(const alpgpu_ctx* ctx, const alpgpu_column* col, int value_bytes) {
	const alpgpu::ColumnSizes sizes {col->n_vectors, col->packed_bytes_hint, col->exc_bytes_hint, alpgpu::policy_rd_vectors_of_hint(col->alp_rd_rowgroups_hint)};
	return alpgpu::policy_decode_plan(sizes, value_bytes, ctx->decode_opt); // (a context always has the progress words the read-ahead needs: alpgpu_ctx_create fails without)
}

// ---- a launch rule that sees more than the column's averages (round 5) -------------------------------------------------------------------------
// alpgpu_column_totals and alpgpu_column_from_blob record, per segment of the column, what they record for the whole: packed bytes, exceptions, ALP_RD
// vectors.  alpgpu_decode_f64 of that column (same context, same descriptor buffer) merges adjacent segments of the same KIND (decode_policy.hpp:
// policy_stretch_kind) into runs and decodes run by run, each through the rule (policy_decode_plan) with the run's own sizes: a column whose first half is
// 6-bit vectors with exceptions and whose second half is 44-bit vectors
// (bench.py: decode_bimodal) gets two vectors per workgroup + the read-ahead for the first and one per workgroup, six workgroups per CU, for the second,
// instead of the shape of their average.  One kind, or more than kMaxRuns runs (a column that changes every few thousand vectors is served by its average): the
// whole column in one launch, as before.  ALPGPU_OPT_DECODE_SEGMENTS = 0: never.  Launch shapes only: the bytes cannot differ.
constexpr int      kMaxRuns           = 8;
struct DecodeRun {
	uint64_t v0, n, packed, exc_bytes, rd_vectors;
};

uint64_t segment_vectors_for(uint64_t n_vectors) {
	uint64_t sv = (n_vectors + kMaxSegments - 1) / kMaxSegments;
	sv          = (sv + 399) / 400 * 400;
	return sv < kSegmentMinVectors ? kSegmentMinVectors : sv;
}

static SegmentTable* segment_table_of(alpgpu_ctx* ctx, const alpgpu_column* col) {
	for (auto& t : ctx->seg_tables) {
		if (t.key != nullptr && t.key == col->d_vectors && t.d_packed == col->d_packed && t.n_vectors == col->n_vectors && t.packed_bytes == col->packed_bytes_hint &&
		    t.exc_bytes == col->exc_bytes_hint) {
			return &t;
		}
	}
	return nullptr;
}
static void segment_tables_drop(alpgpu_ctx* ctx, const alpgpu_column* col) {
	for (auto& t : ctx->seg_tables) {
		if (t.key == col->d_vectors) { t.key = nullptr; }
	}
}
void segment_table_forget(alpgpu_ctx* ctx, const alpgpu_column* col) {
	if (!ctx || !col) { return; }
	segment_tables_drop(ctx, col);
	for (auto& l : ctx->learn) { // ... and what an unhinted decode of the old content left behind (decode_unhinted)
		if (l.state != 0 && l.key == col->d_vectors) {
			// (a copy in flight targets the slot's host words: the slot is abandoned, not waited for — no host synchronisation, and every alpgpu_encode_* comes here,
			//  inside a stream capture too; decode_unhinted takes it again once its event has completed)
			l.state = l.state == 1 ? 3 : 0;
			l.key   = nullptr;
		}
	}
}
// (packed_bytes / exc_bytes: the stream sizes the caller is about to write into the column's hints)
SegmentTable* segment_table_new(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t packed_bytes, uint64_t exc_bytes) {
	segment_tables_drop(ctx, col);
	SegmentTable* t = nullptr;
	for (auto& c : ctx->seg_tables) {
		if (c.key == nullptr) { t = &c; break; }
	}
	if (!t) {
		t             = &ctx->seg_tables[ctx->seg_next];
		ctx->seg_next = (ctx->seg_next + 1) % 4;
	}
	t->key         = col->d_vectors;
	t->d_packed    = col->d_packed;
	t->n_vectors   = col->n_vectors;
	t->packed_bytes = packed_bytes, t->exc_bytes = exc_bytes;
	t->seg_vectors = segment_vectors_for(col->n_vectors);
	t->n_seg       = static_cast<uint32_t>((col->n_vectors + t->seg_vectors - 1) / t->seg_vectors);
	return t;
}

// runs[0 .. return) cover the column; 0 = no plan (decode the column whole)
static int plan_decode_runs(alpgpu_ctx* ctx, const alpgpu_column* col, DecodeRun* runs, int value_bytes) {
	if (!ctx->decode_segments || ctx->decode_opt.forced_vpw != 0 || ctx->decode_opt.forced_pad_kib >= 0) { return 0; } // (a forced shape is a forced shape)
	const SegmentTable* t = segment_table_of(ctx, col);
	if (!t || t->n_seg < 2) { return 0; }
	int n_runs = 0, kind = -1;
	for (uint32_t s = 0; s < t->n_seg; ++s) {
		const uint64_t v0 = s * t->seg_vectors;
		const uint64_t n  = v0 + t->seg_vectors < t->n_vectors ? t->seg_vectors : t->n_vectors - v0;
		const uint64_t eb = (value_bytes + 2ull) * t->exc_cnt[s]; // (ALP: the value + a 2-byte position; ALP_RD records are smaller and their vectors wide anyway)
		const int      k  = alpgpu::policy_stretch_kind(n, t->packed[s], eb, value_bytes);
		if (k != kind) {
			if (n_runs == kMaxRuns) { return 0; }
			runs[n_runs++] = DecodeRun {v0, 0, 0, 0, 0};
			kind           = k;
		}
		DecodeRun& r = runs[n_runs - 1];
		r.n += n, r.packed += t->packed[s], r.exc_bytes += eb, r.rd_vectors += t->rd_vectors[s];
	}
	return n_runs >= 2 ? n_runs : 0;
}

// the view of a run: descriptors hold absolute stream offsets, so a stretch of whole rowgroups decodes on its own
static alpgpu_column run_view(const alpgpu_column* col, const DecodeRun& r) {
	alpgpu_column v   = *col;
	v.n_vectors       = r.n;
	v.n_rowgroups     = (r.n + 99) / 100;
	v.d_vectors       = col->d_vectors + r.v0;
	v.d_rowgroups     = col->d_rowgroups + r.v0 / 100;
	v.packed_bytes_hint = r.packed ? r.packed : 1;
	v.exc_bytes_hint    = r.exc_bytes;
	v.alp_rd_rowgroups_hint = 1 + r.rd_vectors / 100;
	return v;
}

// what alpgpu_decode_f64 / _f32 would launch for this column right now (option + size hints): vectors per decode workgroup
int alpgpu_decode_vectors_per_wg(alpgpu_ctx* ctx, const alpgpu_column* col, int is_f32) {
	if (!ctx || !col) { return fail(ALPGPU_ERR_INVALID, "null context or column"); }
	return alpgpu::decode_shape_number(planned(ctx, col, is_f32 ? 4 : 8).shape);
}

// ... and whether it would start the read-ahead beside the decode kernel (ALPGPU_OPT_DECODE_READ_AHEAD): 1 / 0; negative on bad arguments
int alpgpu_decode_reads_ahead(alpgpu_ctx* ctx, const alpgpu_column* col, int is_f32) {
	if (!ctx || !col) { return fail(ALPGPU_ERR_INVALID, "null context or column"); }
	return planned(ctx, col, is_f32 ? 4 : 8).ahead ? 1 : 0;
}

// measurement aid: what alpgpu_decode_sum_f64 costs with its unpack arithmetic left out (decode_kernels.hip: kSinkProbe)
int alpgpu_debug_decode_probe_f64(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_out) {
	ALPGPU_CHECK_CTX(ctx);
	if (!col || (!d_out && col->n_vectors)) { return fail(ALPGPU_ERR_INVALID, "null column or output"); }
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	if (!col->d_vectors || !col->d_rowgroups) { return fail(ALPGPU_ERR_INVALID, "column has no descriptors"); }
	if (alpgpu::launch_decode_probe(ctx->stream, col, d_out) != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "decode probe launch failed", hipGetLastError()); }
	return ALPGPU_OK;
}
// which kernel computes the per-vector sums (ALPGPU_OPT_CONSUMER_PIPELINED)
// 0 (default) and 2: one wavefront per vector (k_sink_direct) whatever the column holds — ahead of the staged four-wavefront kernel on ALP
// columns (0.81 against 0.91 ms per 1 Mi vectors of the benchmark column) and, since its ALP_RD arm stopped spilling, on ALP_RD columns too
// (1.41 against 1.51 ms); 1: the persistent LDS-ring kernel; 3: the staged four-wavefront kernel.  (alp_rd_rowgroups_hint, which chose
// between the two while the ALP_RD arm spilled, is still kept up to date in the column for callers that want to know.)
// Float columns: the one-wavefront kernel whatever the column holds too (0.99 against 1.08 ms for the staged kernel on the decimal column, 1.04
// against 1.06 on an all-ALP_RD one); options 1 and 3 select the staged kernel (there is no ring kernel).
static bool use_direct_sink(const alpgpu_ctx* ctx) { return ctx->pipelined_consumer == 0 || ctx->pipelined_consumer == 2; }
static int sum_launch(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_sums, bool f32) {
	if (f32) { return use_direct_sink(ctx) ? alpgpu::launch_sink_direct_f32(ctx->stream, col, 0.0f, 0.0f, d_sums, false) : alpgpu::launch_decode_sum_f32(ctx->stream, col, d_sums); }
	if (ctx->pipelined_consumer == 1) { return alpgpu::launch_consume_sum(ctx->stream, col, d_sums, ctx->n_cus); }
	if (use_direct_sink(ctx)) { return alpgpu::launch_sink_direct(ctx->stream, col, 0.0, 0.0, d_sums, false); }
	return alpgpu::launch_decode_sum(ctx->stream, col, d_sums, 2);
}

static int decode_sum(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_sums, bool f32) {
	ALPGPU_CHECK_CTX(ctx);
	if (!col || (!d_sums && col->n_vectors)) { return fail(ALPGPU_ERR_INVALID, "null column or output"); }
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	if (!col->d_vectors || !col->d_rowgroups) { return fail(ALPGPU_ERR_INVALID, "column has no descriptors"); }
	if (sum_launch(ctx, col, d_sums, f32) != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "decode-sum launch failed", hipGetLastError()); }
	return ALPGPU_OK;
}
int alpgpu_decode_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_sums) { return decode_sum(ctx, col, d_sums, false); }
int alpgpu_decode_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_sums) { return decode_sum(ctx, col, d_sums, true); }

// The whole column's total (the reference's consumer keeps ONE accumulator across vectors, q1.cpp:91-100): per-vector sums into the
// context's workspace, then the documented tree over them.  Everything stays on the stream; *d_total is device memory.
static int column_sum(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_total, bool f32) {
	ALPGPU_CHECK_CTX(ctx);
	if (!col || !d_total) { return fail(ALPGPU_ERR_INVALID, "null column or output"); }
	const uint64_t n = col->n_vectors;
	if (n == 0) {
		ALPGPU_HIP(hipMemsetAsync(d_total, 0, sizeof(double), ctx->stream));
		return ALPGPU_OK;
	}
	if (!col->d_vectors || !col->d_rowgroups) { return fail(ALPGPU_ERR_INVALID, "column has no descriptors"); }
	const uint64_t l1 = (n + 1023) / 1024;
	if (int rc = ensure_workspace(ctx, 8ull * (n + 2 * l1) + 64)) { return rc; }
	double* sums = static_cast<double*>(ctx->workspace);
	int     rc   = sum_launch(ctx, col, sums, f32);
	if (rc == ALPGPU_OK) { rc = alpgpu::launch_tree_sum(ctx->stream, sums, n, sums + n, d_total); }
	if (rc != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "column-sum launch failed", hipGetLastError()); }
	return workspace_used(ctx);
}
int alpgpu_column_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_total) { return column_sum(ctx, col, d_total, false); }
int alpgpu_column_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_total) { return column_sum(ctx, col, d_total, true); }
// the same tree over any device array of doubles (e.g. the per-vector sums a caller already has)
int alpgpu_tree_sum_f64(alpgpu_ctx* ctx, const double* d_in, uint64_t n, double* d_total) {
	ALPGPU_CHECK_CTX(ctx);
	if ((!d_in && n) || !d_total) { return fail(ALPGPU_ERR_INVALID, "null input or output"); }
	const uint64_t l1 = (n + 1023) / 1024;
	if (int rc = ensure_workspace(ctx, 16ull * l1 + 64)) { return rc; }
	if (alpgpu::launch_tree_sum(ctx->stream, d_in, n, static_cast<double*>(ctx->workspace), d_total) != ALPGPU_OK) {
		return fail(ALPGPU_ERR_HIP, "tree-sum launch failed", hipGetLastError());
	}
	return workspace_used(ctx);
}

// (a float column's bounds are floats: they pass through double unchanged)
static int decode_count_range(alpgpu_ctx* ctx, const alpgpu_column* col, double lo, double hi, uint32_t* d_counts, bool f32) {
	ALPGPU_CHECK_CTX(ctx);
	if (!col || (!d_counts && col->n_vectors)) { return fail(ALPGPU_ERR_INVALID, "null column or output"); }
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	if (!col->d_vectors || !col->d_rowgroups) { return fail(ALPGPU_ERR_INVALID, "column has no descriptors"); }
	const float flo = static_cast<float>(lo), fhi = static_cast<float>(hi);
	const int   rc  = f32 ? (use_direct_sink(ctx) ? alpgpu::launch_sink_direct_f32(ctx->stream, col, flo, fhi, d_counts, true) : alpgpu::launch_decode_count_range_f32(ctx->stream, col, flo, fhi, d_counts))
	                : ctx->pipelined_consumer == 1 ? alpgpu::launch_consume_count_range(ctx->stream, col, lo, hi, d_counts, ctx->n_cus)
	                : use_direct_sink(ctx)         ? alpgpu::launch_sink_direct(ctx->stream, col, lo, hi, d_counts, true)
	                                               : alpgpu::launch_decode_count_range(ctx->stream, col, lo, hi, d_counts);
	if (rc != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "decode-count launch failed", hipGetLastError()); }
	return ALPGPU_OK;
}
int alpgpu_decode_count_range_f64(alpgpu_ctx* ctx, const alpgpu_column* col, double lo, double hi, uint32_t* d_counts) { return decode_count_range(ctx, col, lo, hi, d_counts, false); }
int alpgpu_decode_count_range_f32(alpgpu_ctx* ctx, const alpgpu_column* col, float lo, float hi, uint32_t* d_counts) { return decode_count_range(ctx, col, lo, hi, d_counts, true); }

extern "C++" {
// the next tag of the context's progress word (its top 24 bits: a stale value of an earlier launch reads as "not started")
static uint64_t next_progress_tag(alpgpu_ctx* ctx) {
	ctx->progress_gen = (ctx->progress_gen + 1) & 0xFFFFFFull;
	if (ctx->progress_gen == 0) { ctx->progress_gen = 1; }
	return ctx->progress_gen << 40;
}

// one launch of the store decode over a column or a run of it (+ the read-ahead beside it where the rule wants one); VB = 8 (double) or 4 (float)
template <int VB>
static int decode_one(alpgpu_ctx* ctx, const alpgpu_column* col, void* d_out) {
	// The read-ahead (read_ahead_kernels.hip): a few persistent workgroups on the context's second stream pull the column's streams into the Infinity
	// Cache a bounded distance ahead of the decode kernel, which tells them where it is.  Started first so that it is ahead from the first workgroup on.
	// (a float column streamed by persistent workgroups prefetches for itself; the read-ahead beside it changed nothing: call 14)
	const alpgpu::DecodePlan plan  = planned(ctx, col, VB);
	const bool               ahead = plan.ahead;
	uint64_t                 tag   = 0;
	if (ahead) {
		tag = next_progress_tag(ctx);
		ALPGPU_HIP(hipEventRecord(ctx->ev_fork, ctx->stream)); // (the read-ahead may start where the decode may)
	}
	// The decode kernel is enqueued FIRST (round 6; until round 5 the read-ahead was): whatever delays the host between the two launches — the lazy load of a code
	// object on a process's first decode takes milliseconds — then costs the read-ahead a late start instead of its patience (a read-ahead that waits for a decode
	// that is not even enqueued leaves, and that decode then runs without one).  The side stream has the higher priority: its few workgroups are placed at once.
	int rc;
	if constexpr (VB == 8) {
		rc = alpgpu::launch_decode_column(ctx->stream, col, static_cast<double*>(d_out), plan.shape, ctx->n_cus, ahead ? ctx->d_progress : nullptr, tag);
	} else if (plan.shape.family == alpgpu::kDecodeStreamed) { // persistent workgroups (decode_stream_f32_kernels.hip): no read-ahead beside it, nothing to report
		rc = alpgpu::launch_decode_stream_f32(ctx->stream, col, static_cast<float*>(d_out), plan.shape.stream_shape, ctx->n_cus, nullptr, 0);
	} else {
		rc = alpgpu::launch_decode_column_f32(ctx->stream, col, static_cast<float*>(d_out), plan.shape, ahead ? ctx->d_progress : nullptr, tag);
	}
	if (ahead) {
		const alpgpu::ReadAheadPace pace = alpgpu::policy_read_ahead_pace(static_cast<double>(col->n_vectors), static_cast<double>(col->packed_bytes_hint),
		                                                                  static_cast<double>(col->exc_bytes_hint), VB, ctx->read_ahead_us); // (decode_policy.hpp: the lead is a time)
		ALPGPU_HIP(hipStreamWaitEvent(ctx->init_stream, ctx->ev_fork, 0));
		if (alpgpu::launch_read_ahead(ctx->init_stream, col, VB, ctx->d_progress, tag, pace.lead_min, pace.lead_max, pace.ps_per_vector, ctx->wall_tick_ps, kReadAheadMaxBits, kReadAheadGrid) != ALPGPU_OK) {
			return fail(ALPGPU_ERR_HIP, "read-ahead launch failed", hipGetLastError());
		}
		ALPGPU_HIP(hipEventRecord(ctx->ev_join, ctx->init_stream));
	}
	if (ahead) { ALPGPU_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0)); } // (the read-ahead leaves on its own once its last batch is in reach or the decode never shows up)
	if (rc != ALPGPU_OK) { return fail(rc, "decode launch failed", hipGetLastError()); }
	return ALPGPU_OK;
}

// ---- a column whose sizes the host does not know (round 6) ------------------------------------------------------------------------
// alpgpu_encode_* leaves the stream sizes in device memory; the host learns them from alpgpu_column_totals, a synchronisation.  A caller that encodes and
// decodes without it used to get one vector per workgroup and no read-ahead (0.50 on 4-bit vectors where the hinted decode reaches 0.72-0.76).  Now, for columns of
// at least kUnhintedMinVectors vectors: the per-segment sums are taken on the stream (k_segment_sums, 17 us per 1 Mi vectors), k_unhinted_plan evaluates the rule on
// the device (decode_policy.hpp) and the read-ahead beside the decode takes its lead and pace — or "not for this column" — from the plan's words.  The sums also
// travel to page-locked host memory behind an event nobody waits for: the NEXT decode of the same column (same descriptor and packed buffers, same length, not
// encoded again in between) finds them there and is planned on the host like a hinted one, launch shape and regions included (call 1b: 1.00-1.05 of the hinted
// figure from the second decode on).  The launch shape of the FIRST decode: see decode_unhinted.  ALPGPU_OPT_DECODE_UNHINTED = 0: the old behaviour.
constexpr uint64_t kUnhintedMinVectors = 65536;

static LearnSlot* learn_slot_of(alpgpu_ctx* ctx, const alpgpu_column* col, int value_bytes) {
	for (auto& l : ctx->learn) {
		if ((l.state == 1 || l.state == 2) && l.key == col->d_vectors && l.d_packed == col->d_packed && l.n_vectors == col->n_vectors && l.value_bytes == value_bytes) { return &l; }
	}
	return nullptr;
}

// the column with the sizes an earlier unhinted decode of it left behind, if they have arrived; false: nothing known (yet)
static bool learned_hints(alpgpu_ctx* ctx, const alpgpu_column* col, int value_bytes, alpgpu_column* hinted) {
	LearnSlot* l = learn_slot_of(ctx, col, value_bytes);
	if (!l) { return false; }
	if (l->state == 1) {
		if (hipEventQuery(l->ev) != hipSuccess) {
			(void)hipGetLastError(); // not ready: not an error
			return false;
		}
		const uint64_t* sums = ctx->h_learn + static_cast<size_t>(l - ctx->learn) * 3 * kMaxSegments;
		l->packed = l->exceptions = l->rd_vectors = 0;
		for (uint32_t i = 0; i < l->n_seg; ++i) { l->packed += sums[3 * i], l->exceptions += sums[3 * i + 1], l->rd_vectors += sums[3 * i + 2]; }
		l->state = 2;
		if (l->n_seg >= 2) { // the decode's launch plan (plan_decode_runs), as alpgpu_column_totals would have left it
			alpgpu_column c = *col;
			SegmentTable* t = segment_table_new(ctx, &c, l->packed ? l->packed : 1, (value_bytes + 2ull) * l->exceptions);
			for (uint32_t i = 0; i < t->n_seg && i < l->n_seg; ++i) { t->packed[i] = sums[3 * i], t->exc_cnt[i] = sums[3 * i + 1], t->rd_vectors[i] = sums[3 * i + 2]; }
		}
	}
	*hinted = *col;
	hinted->packed_bytes_hint     = l->packed ? l->packed : 1; // (a column of nothing but 0-bit vectors: "known, and narrow")
	hinted->exc_bytes_hint        = (value_bytes + 2ull) * l->exceptions;
	hinted->alp_rd_rowgroups_hint = 1 + l->rd_vectors / 100;
	return true;
}

// (learn = false: the stream is capturing — the sums are not sent anywhere)
template <int VB>
static int decode_unhinted(alpgpu_ctx* ctx, const alpgpu_column* col, void* d_out, bool learn) {
	uint64_t* words = ctx->d_progress;
	const uint64_t seg_vectors = segment_vectors_for(col->n_vectors);
	const uint32_t n_seg       = static_cast<uint32_t>((col->n_vectors + seg_vectors - 1) / seg_vectors);
	if (alpgpu::launch_segment_sums(ctx->stream, col, seg_vectors, n_seg, words + alpgpu::kCtxWordSegments) != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "segment sums launch failed", hipGetLastError()); }
	if (alpgpu::launch_unhinted_plan(ctx->stream, words, n_seg, col->n_vectors, VB, (ctx->decode_opt.read_ahead < 0 && ctx->decode_opt.streams_serialize) ? 0 : ctx->decode_opt.read_ahead, ctx->read_ahead_us, kReadAheadMaxBits) != ALPGPU_OK) {
		return fail(ALPGPU_ERR_HIP, "plan launch failed", hipGetLastError());
	}
	const uint64_t tag        = next_progress_tag(ctx);
	const bool     with_ahead = ctx->decode_opt.read_ahead > 0 || (ctx->decode_opt.read_ahead < 0 && !ctx->decode_opt.streams_serialize);
	if (with_ahead) { ALPGPU_HIP(hipEventRecord(ctx->ev_fork, ctx->stream)); }
	int rc = ALPGPU_OK;
	// Which launch.  A closed candidate is not free: the dispatcher hands out ~5.5 workgroups per nanosecond, so 1 Mi empty workgroups cost 0.19 ms — 10-17 % of a
	// decode (call 1b: first unhinted decode 0.59-0.68 of peak against 0.72-0.81 hinted with all three candidates launched).  Default (1) therefore: ONE launch in the
	// shape a column without hints always got (the first candidate — double: one vector per workgroup, 6 KiB pad; float: two), un-gated, and the device-side plan steers
	// the read-ahead only — which is what narrow columns gain most from — while the sizes travel to the host for the next decode.  2: every candidate, gated (the
	// measured alternative).  The candidates: decode_policy.hpp, beside policy_unhinted, which numbers them.
	const int n_launch = ctx->decode_unhinted == 2 ? (VB == 8 ? alpgpu::kUnhintedShapesF64 : alpgpu::kUnhintedShapesF32) : 1;
	for (int c = 0; c < n_launch && rc == ALPGPU_OK; ++c) {
		alpgpu::DecodeShape shape = VB == 8 ? alpgpu::kUnhintedCandidatesF64[c] : alpgpu::kUnhintedCandidatesF32[c];
		shape.plain_stores        = ctx->decode_opt.plain_stores;
		const uint32_t gate       = n_launch > 1 ? static_cast<uint32_t>(c + 1) : 0u;
		rc = VB == 8 ? alpgpu::launch_decode_column(ctx->stream, col, static_cast<double*>(d_out), shape, ctx->n_cus, words, tag, gate)
		             : alpgpu::launch_decode_column_f32(ctx->stream, col, static_cast<float*>(d_out), shape, words, tag, gate);
	}
	if (with_ahead) { // behind the decode's launch (decode_one says why); the kernel leaves at once when the plan says "no read-ahead for this column"
		ALPGPU_HIP(hipStreamWaitEvent(ctx->init_stream, ctx->ev_fork, 0));
		if (alpgpu::launch_read_ahead(ctx->init_stream, col, VB, words, tag, 0, 0, 0, ctx->wall_tick_ps, 0, kReadAheadGrid, true) != ALPGPU_OK) {
			return fail(ALPGPU_ERR_HIP, "read-ahead launch failed", hipGetLastError());
		}
		ALPGPU_HIP(hipEventRecord(ctx->ev_join, ctx->init_stream));
	}
	// the sums, for the next decode of this column: to page-locked memory behind an event that is only ever queried (enqueued BEHIND the decode: the copy delays nothing)
	if (learn && ctx->h_learn != nullptr) {
		LearnSlot* l = learn_slot_of(ctx, col, VB);
		if (!l) {
			l               = &ctx->learn[ctx->learn_next];
			ctx->learn_next = (ctx->learn_next + 1) % kLearnSlots;
		}
		// (a slot whose copy is still in flight — the same column decoded again before its sizes arrived, or a fifth unhinted column within microseconds — is left
		//  alone: no host synchronisation here either; the earlier copy lands, or this column simply stays unhinted a little longer)
		const bool busy = (l->state == 1 || l->state == 3) && hipEventQuery(l->ev) != hipSuccess;
		if (busy) {
			(void)hipGetLastError();
		} else {
			l->key = col->d_vectors, l->d_packed = col->d_packed, l->n_vectors = col->n_vectors, l->value_bytes = VB, l->n_seg = n_seg;
			l->state = 0;
			if (hipMemcpyAsync(ctx->h_learn + static_cast<size_t>(l - ctx->learn) * 3 * kMaxSegments, words + alpgpu::kCtxWordSegments, 24ull * n_seg, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
			    hipEventRecord(l->ev, ctx->stream) == hipSuccess) {
				l->state = 1;
			} else {
				(void)hipGetLastError(); // best effort: the column simply stays unhinted
			}
		}
	}
	if (with_ahead) { ALPGPU_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0)); }
	if (rc != ALPGPU_OK) { return fail(rc, "decode launch failed", hipGetLastError()); }
	return ALPGPU_OK;
}

// the column's sizes are unknown to the host and the decode takes them on the stream (decode_unhinted), or from what an earlier one learned
static bool decodes_unhinted(const alpgpu_ctx* ctx, const alpgpu_column* col, int value_bytes) {
	const bool unhinted   = col->packed_bytes_hint == 0 && col->exc_bytes_hint == 0;
	const bool free_shape = ctx->decode_opt.forced_vpw == 0 && ctx->decode_opt.forced_pad_kib < 0;
	return unhinted && ctx->decode_unhinted && free_shape && ctx->d_progress != nullptr && col->n_vectors >= kUnhintedMinVectors;
}
static bool stream_capturing(hipStream_t s) {
	hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
	if (hipStreamIsCapturing(s, &st) != hipSuccess) {
		(void)hipGetLastError();
		return true; // (cannot tell: the learn slots are left alone)
	}
	return st != hipStreamCaptureStatusNone;
}

template <int VB>
static int decode_column(alpgpu_ctx* ctx, const alpgpu_column* col, void* d_out) {
	ALPGPU_CHECK_CTX(ctx);
	if (!col || (!d_out && col->n_vectors)) { return fail(ALPGPU_ERR_INVALID, "null column or output"); }
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	if (!col->d_vectors || !col->d_rowgroups) { return fail(ALPGPU_ERR_INVALID, "column has no descriptors"); }
	alpgpu_column hinted;
	if (decodes_unhinted(ctx, col, VB)) {
		// Captured into a graph: the device-side plan only.  A slot's event recorded and its copy made only in a capture would be queried by the next eager decode
		// before any replay wrote the host words (and every replay would write them again behind the host's back).
		if (stream_capturing(ctx->stream)) { return decode_unhinted<VB>(ctx, col, d_out, false); }
		if (learned_hints(ctx, col, VB, &hinted)) {
			col = &hinted; // an earlier decode of this column took its sizes: planned on the host from here on
		} else {
			return decode_unhinted<VB>(ctx, col, d_out, true);
		}
	}
	DecodeRun runs[kMaxRuns];
	const int n_runs = plan_decode_runs(ctx, col, runs, VB);
	if (n_runs == 0) { return decode_one<VB>(ctx, col, d_out); }
	for (int i = 0; i < n_runs; ++i) { // regions of different kinds, each with its own launch shape (plan_decode_runs)
		const alpgpu_column view = run_view(col, runs[i]);
		if (const int rc = decode_one<VB>(ctx, &view, static_cast<uint8_t*>(d_out) + runs[i].v0 * 1024 * VB)) { return rc; }
	}
	return ALPGPU_OK;
}
} // extern "C++"

int alpgpu_decode_f64(alpgpu_ctx* ctx, const alpgpu_column* col, double* d_out) { return decode_column<8>(ctx, col, d_out); }
int alpgpu_decode_f32(alpgpu_ctx* ctx, const alpgpu_column* col, float* d_out) { return decode_column<4>(ctx, col, d_out); }

// debug aids (tests): batches of 64 vectors the context's read-aheads have read so far; the plan words of its last unhinted decode
// (out[0] shape, [1] lead_min | lead_max << 32, [2] ps per vector | max bits << 32, [3..5] packed bytes, exceptions, ALP_RD vectors).  Both wait for the stream.
int alpgpu_debug_read_ahead_batches(alpgpu_ctx* ctx, uint64_t* batches) {
	ALPGPU_CHECK_CTX(ctx);
	if (!batches || !ctx->d_progress) { return fail(ALPGPU_ERR_INVALID, "null output"); }
	ALPGPU_HIP(hipStreamSynchronize(ctx->stream));
	ALPGPU_HIP(hipStreamSynchronize(ctx->init_stream));
	ALPGPU_HIP(hipMemcpy(batches, ctx->d_progress + alpgpu::kCtxWordBatches, 8, hipMemcpyDeviceToHost));
	return ALPGPU_OK;
}
int alpgpu_debug_forget_column(alpgpu_ctx* ctx, const alpgpu_column* col) {
	ALPGPU_CHECK_CTX(ctx);
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	segment_table_forget(ctx, col);
	return ALPGPU_OK;
}
int alpgpu_debug_unhinted_plan(alpgpu_ctx* ctx, uint64_t* out6) {
	ALPGPU_CHECK_CTX(ctx);
	if (!out6 || !ctx->d_progress) { return fail(ALPGPU_ERR_INVALID, "null output"); }
	ALPGPU_HIP(hipStreamSynchronize(ctx->stream));
	uint64_t w[16];
	ALPGPU_HIP(hipMemcpy(w, ctx->d_progress, sizeof(w), hipMemcpyDeviceToHost));
	out6[0] = w[alpgpu::kCtxWordShape], out6[1] = w[alpgpu::kCtxWordLead], out6[2] = w[alpgpu::kCtxWordPace];
	out6[3] = w[alpgpu::kCtxWordTotals], out6[4] = w[alpgpu::kCtxWordTotals + 1], out6[5] = w[alpgpu::kCtxWordTotals + 2];
	return ALPGPU_OK;
}

// debug aid (tests): the launch decode() of this column would make now, for the column as a whole (a region plan gives each run its own: alpgpu_decode_runs).
// out4[0] the shape as the word include/alpgpu.h documents (decode_policy.hpp: decode_debug_word); [1..3] the sizes it is planned from
// (packed_bytes_hint, exc_bytes_hint, alp_rd_rowgroups_hint — for an unhinted column, what an earlier decode of it learned).  Returns 1: planned on the host; 0: an
// unhinted decode whose plan is made on the device (out4 untouched); negative on bad arguments.  Waits for nothing.
int alpgpu_debug_decode_plan(alpgpu_ctx* ctx, const alpgpu_column* col, int is_f32, uint64_t* out4) {
	ALPGPU_CHECK_CTX(ctx); // (learned_hints queries an event)
	if (!col || !out4) { return fail(ALPGPU_ERR_INVALID, "null column or output"); }
	alpgpu_column hinted;
	if (decodes_unhinted(ctx, col, is_f32 ? 4 : 8)) {
		if (!learned_hints(ctx, col, is_f32 ? 4 : 8, &hinted)) { return 0; }
		col = &hinted;
	}
	out4[0] = alpgpu::decode_debug_word(planned(ctx, col, is_f32 ? 4 : 8).shape, is_f32 ? 4 : 8);
	out4[1] = col->packed_bytes_hint, out4[2] = col->exc_bytes_hint, out4[3] = col->alp_rd_rowgroups_hint;
	return 1;
}

// how many launches alpgpu_decode_f64 would make for this column now: 1, or the number of runs of plan_decode_runs; negative on bad arguments
static int decode_runs(alpgpu_ctx* ctx, const alpgpu_column* col, int value_bytes) {
	if (!ctx || !col) { return fail(ALPGPU_ERR_INVALID, "null context or column"); }
	DecodeRun runs[kMaxRuns];
	const int n_runs = plan_decode_runs(ctx, col, runs, value_bytes);
	return n_runs == 0 ? 1 : n_runs;
}
int alpgpu_decode_runs(alpgpu_ctx* ctx, const alpgpu_column* col) { return decode_runs(ctx, col, 8); }
int alpgpu_decode_runs_f32(alpgpu_ctx* ctx, const alpgpu_column* col) { return decode_runs(ctx, col, 4); }
int alpgpu_column_totals(alpgpu_ctx* ctx, alpgpu_column* col, uint64_t* packed_bytes, uint64_t* exc_bytes, int* overflow) {
	ALPGPU_CHECK_CTX(ctx);
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	uint64_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	if (col->d_totals) {
		const bool count_rd = col->d_rowgroups != nullptr && col->n_rowgroups != 0;
		if (count_rd && alpgpu::launch_count_rd_rowgroups(ctx->stream, col, col->d_totals + 7) != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "rowgroup count launch failed", hipGetLastError()); }
		// per-segment sums for the decode's launch plan (plan_decode_runs): columns long enough to have two segments
		// (the table is filled first and gets its key last: an early return leaves no half-made entry that a later decode could match — ADVICE round 5)
		uint64_t seg_sums[3 * kMaxSegments];
		uint64_t seg_vectors = 0;
		uint32_t n_seg       = 0;
		segment_table_forget(ctx, col);
		if (col->d_vectors && ctx->d_progress && col->n_vectors >= 2 * kSegmentMinVectors) {
			seg_vectors = segment_vectors_for(col->n_vectors);
			n_seg       = static_cast<uint32_t>((col->n_vectors + seg_vectors - 1) / seg_vectors);
			if (alpgpu::launch_segment_sums(ctx->stream, col, seg_vectors, n_seg, ctx->d_progress + alpgpu::kCtxWordSegments) != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "segment sums launch failed", hipGetLastError()); }
			ALPGPU_HIP(hipMemcpyAsync(seg_sums, ctx->d_progress + alpgpu::kCtxWordSegments, 24ull * n_seg, hipMemcpyDeviceToHost, ctx->stream));
		}
		ALPGPU_HIP(hipMemcpyAsync(t, col->d_totals, sizeof(t), hipMemcpyDeviceToHost, ctx->stream));
		ALPGPU_HIP(hipStreamSynchronize(ctx->stream));
		if (n_seg != 0 && !t[2] && !t[3]) { // (an overflowed or unrecovered column: no plans)
			SegmentTable* seg = segment_table_new(ctx, col, t[0], t[1]);
			for (uint32_t i = 0; i < seg->n_seg && i < n_seg; ++i) { seg->packed[i] = seg_sums[3 * i], seg->exc_cnt[i] = seg_sums[3 * i + 1], seg->rd_vectors[i] = seg_sums[3 * i + 2]; }
		}
		col->alp_rd_rowgroups_hint = count_rd ? 1 + t[7] : (col->n_vectors == 0 ? 1 : 0);
	} else if (col->n_vectors != 0) {
		return fail(ALPGPU_ERR_INVALID, "column without d_totals");
	}
	if (packed_bytes) { *packed_bytes = t[0]; }
	if (exc_bytes) { *exc_bytes = t[1]; }
	if (overflow) { *overflow = static_cast<int>(t[2]); }
	col->packed_bytes_hint = t[0];
	col->exc_bytes_hint    = t[1];
	// cannot happen through alpgpu_encode_*: the recovery route clears the flag (alpgpu_encode_vectors_f64)
	if (t[3]) { return fail(ALPGPU_ERR_HIP, "single-pass encode stalled in its offset look-back and was not recovered"); }
	return t[2] ? fail(ALPGPU_ERR_CAPACITY, "an output stream overflowed its capacity") : ALPGPU_OK;
}
} // extern "C"
