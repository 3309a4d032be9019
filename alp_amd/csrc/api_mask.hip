// api_mask.hip — selection bitmaps of include/alpgpu.h: alpgpu_select_mask_* (a range predicate's qualify mask, set into or combined with a caller's
// bitmap), alpgpu_mask_to_indices (its set bits as ascending value indices), alpgpu_decode_sum_masked_* (per-vector sums of the values whose bit is
// set) and alpgpu_decode_masked_* (those values themselves, compacted).  A call is a handful of launches of mask_kernels.hip on the context's stream and nothing else: no host synchronisation, no second stream, no
// allocation, and none of what the context remembers about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
static int select_mask(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, double lo, double hi, int op, uint64_t* d_mask, int value_bytes) {
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	ALPGPU_TRY(check_mask_op(op));
	ALPGPU_TRY(check_n_vectors(col->n_vectors, "column.n_vectors is implausible"));
	ALPGPU_TRY(check_value_range(col->n_vectors, first, n, "range reaches past the column's last value"));
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	if (!d_mask) { return fail(ALPGPU_ERR_INVALID, "null bitmap"); }
	if (n == 0) { return clear_bitmap_for_empty_range(ctx, op, d_mask, col); }
	ALPGPU_TRY(check_has_descriptors(col));
	const int rc = alpgpu::launch_select_mask(ctx->stream, col, first, n, lo, hi, op, d_mask, value_bytes);
	if (rc != ALPGPU_OK) { return fail(rc, "select_mask launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}

static int sum_masked(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts, int value_bytes) {
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	if (!d_mask || !d_sums) { return fail(ALPGPU_ERR_INVALID, "null bitmap or sums"); }
	ALPGPU_TRY(check_n_vectors(col->n_vectors, "column.n_vectors is implausible"));
	ALPGPU_TRY(check_has_descriptors(col));
	const int rc = alpgpu::launch_sum_masked(ctx->stream, col, d_mask, d_sums, d_counts, value_bytes);
	if (rc != ALPGPU_OK) { return fail(rc, "decode_sum_masked launch failed"); }
	return ALPGPU_OK;
}

static int decode_masked(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, void* d_vals, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch,
                         int value_bytes) {
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (!d_count) { return fail(ALPGPU_ERR_INVALID, "null count"); }
	if (!d_mask) { return fail(ALPGPU_ERR_INVALID, "null bitmap"); }
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	if (capacity > 0 && !d_vals) { return fail(ALPGPU_ERR_INVALID, "null value output with a capacity"); }
	ALPGPU_TRY(check_n_vectors(col->n_vectors, "column.n_vectors is implausible"));
	if (col->n_vectors == 0) { // no bit at all: the count alone is written
		ALPGPU_HIP(hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
		return ALPGPU_OK;
	}
	if (!d_scratch || misaligned(d_scratch, 16u)) { return fail(ALPGPU_ERR_INVALID, "scratch is null or not 16-byte aligned"); }
	ALPGPU_TRY(check_has_descriptors(col));
	const int rc = alpgpu::launch_decode_masked(ctx->stream, col, d_mask, d_vals, d_idx, capacity, d_count, d_scratch, value_bytes);
	if (rc != ALPGPU_OK) { return fail(rc, "decode_masked launch failed"); }
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

int alpgpu_select_mask_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, double lo, double hi, int op, uint64_t* d_mask) {
	ALPGPU_CHECK_CTX(ctx);
	return select_mask(ctx, col, first, n, lo, hi, op, d_mask, 8);
}
int alpgpu_select_mask_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, float lo, float hi, int op, uint64_t* d_mask) {
	ALPGPU_CHECK_CTX(ctx);
	return select_mask(ctx, col, first, n, lo, hi, op, d_mask, 4);
}

int alpgpu_mask_to_indices(alpgpu_ctx* ctx, const uint64_t* d_mask, uint64_t n_vectors, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	if (!d_count) { return fail(ALPGPU_ERR_INVALID, "null count"); }
	ALPGPU_TRY(check_n_vectors(n_vectors, "n_vectors is implausible"));
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	if (capacity > 0 && !d_idx) { return fail(ALPGPU_ERR_INVALID, "null index output with a capacity"); }
	if (n_vectors == 0) { // no bit at all: the count alone is written
		ALPGPU_HIP(hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
		return ALPGPU_OK;
	}
	if (!d_mask) { return fail(ALPGPU_ERR_INVALID, "null bitmap"); }
	if (!d_scratch || misaligned(d_scratch, 16u)) { return fail(ALPGPU_ERR_INVALID, "scratch is null or not 16-byte aligned"); }
	const int rc = alpgpu::launch_mask_to_indices(ctx->stream, d_mask, n_vectors, d_idx, capacity, d_count, d_scratch);
	if (rc != ALPGPU_OK) { return fail(rc, "mask_to_indices launch failed"); }
	return ALPGPU_OK;
}

int alpgpu_decode_sum_masked_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	return sum_masked(ctx, col, d_mask, d_sums, d_counts, 8);
}
int alpgpu_decode_sum_masked_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	return sum_masked(ctx, col, d_mask, d_sums, d_counts, 4);
}

int alpgpu_decode_masked_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, double* d_vals, int64_t* d_idx, uint64_t capacity, uint64_t* d_count,
                             void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return decode_masked(ctx, col, d_mask, d_vals, d_idx, capacity, d_count, d_scratch, 8);
}
int alpgpu_decode_masked_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, float* d_vals, int64_t* d_idx, uint64_t capacity, uint64_t* d_count,
                             void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return decode_masked(ctx, col, d_mask, d_vals, d_idx, capacity, d_count, d_scratch, 4);
}

} // extern "C"
