// api_pair.hip — two-column consumers of include/alpgpu.h: alpgpu_compare_mask_* (a_r CMP b_r between two columns of equal length, set into or
// combined with a caller's bitmap) and alpgpu_decode_dot_masked_* (per-vector sums of a_r * b_r over the set bits).  A call is one launch of
// pair_kernels.hip on the context's stream and nothing else: no host synchronisation, no second stream, no allocation, and none of what the
// context remembers about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
// what both entry points ask of their columns and bitmap
static int check_pair(const alpgpu_column* a, const alpgpu_column* b, const void* d_mask) {
	if (!a || !b) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (a->n_vectors != b->n_vectors) { return fail(ALPGPU_ERR_INVALID, "the columns differ in n_vectors"); }
	ALPGPU_TRY(check_n_vectors(a->n_vectors, "column.n_vectors is implausible"));
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	return ALPGPU_OK;
}

static int compare_mask(alpgpu_ctx* ctx, const alpgpu_column* a, const alpgpu_column* b, uint64_t first, uint64_t n, int cmp, int op, uint64_t* d_mask, int value_bytes) {
	if (cmp < ALPGPU_CMP_LT || cmp > ALPGPU_CMP_NE) { return fail(ALPGPU_ERR_INVALID, "cmp is none of ALPGPU_CMP_LT .. _NE"); }
	ALPGPU_TRY(check_mask_op(op));
	const int ok = check_pair(a, b, d_mask);
	if (ok != ALPGPU_OK) { return ok; }
	ALPGPU_TRY(check_value_range(a->n_vectors, first, n, "range reaches past the columns' last value"));
	if (a->n_vectors == 0) { return ALPGPU_OK; }
	if (!d_mask) { return fail(ALPGPU_ERR_INVALID, "null bitmap"); }
	if (n == 0) { return clear_bitmap_for_empty_range(ctx, op, d_mask, a); }
	ALPGPU_TRY(check_has_descriptors(a, b));
	const int rc = alpgpu::launch_compare_mask(ctx->stream, a, b, first, n, cmp, op, d_mask, value_bytes);
	if (rc != ALPGPU_OK) { return fail(rc, "compare_mask launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}

static int dot_masked(alpgpu_ctx* ctx, const alpgpu_column* a, const alpgpu_column* b, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts, int value_bytes) {
	const int ok = check_pair(a, b, d_mask);
	if (ok != ALPGPU_OK) { return ok; }
	if (a->n_vectors == 0) { return ALPGPU_OK; }
	if (!d_mask || !d_sums) { return fail(ALPGPU_ERR_INVALID, "null bitmap or sums"); }
	ALPGPU_TRY(check_has_descriptors(a, b));
	const int rc = alpgpu::launch_dot_masked(ctx->stream, a, b, d_mask, d_sums, d_counts, value_bytes);
	if (rc != ALPGPU_OK) { return fail(rc, "decode_dot_masked launch failed"); }
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

int alpgpu_compare_mask_f64(alpgpu_ctx* ctx, const alpgpu_column* a, const alpgpu_column* b, uint64_t first, uint64_t n, int cmp, int op, uint64_t* d_mask) {
	ALPGPU_CHECK_CTX(ctx);
	return compare_mask(ctx, a, b, first, n, cmp, op, d_mask, 8);
}
int alpgpu_compare_mask_f32(alpgpu_ctx* ctx, const alpgpu_column* a, const alpgpu_column* b, uint64_t first, uint64_t n, int cmp, int op, uint64_t* d_mask) {
	ALPGPU_CHECK_CTX(ctx);
	return compare_mask(ctx, a, b, first, n, cmp, op, d_mask, 4);
}

int alpgpu_decode_dot_masked_f64(alpgpu_ctx* ctx, const alpgpu_column* a, const alpgpu_column* b, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	return dot_masked(ctx, a, b, d_mask, d_sums, d_counts, 8);
}
int alpgpu_decode_dot_masked_f32(alpgpu_ctx* ctx, const alpgpu_column* a, const alpgpu_column* b, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	return dot_masked(ctx, a, b, d_mask, d_sums, d_counts, 4);
}

} // extern "C"
