// api_minmax.hip — masked and grouped MIN / MAX of include/alpgpu.h: alpgpu_decode_minmax_masked_* (one {min, max} record per vector over the
// values a bitmap selects), alpgpu_decode_group_minmax_* (the same per closed range of a key column, up to ALPGPU_GROUP_MAX groups in one pass) and
// alpgpu_group_minmax_totals_* (every group's column MIN / MAX).  A call is launches of minmax_kernels.hip on the context's stream and nothing
// else: no host synchronisation, no second stream, no allocation, the context's workspace is not used and none of what the context remembers
// about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
static int minmax_masked(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, void* d_zones, uint32_t* d_counts, int value_bytes) {
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	if (misaligned(d_zones, 2u * value_bytes)) { return fail(ALPGPU_ERR_INVALID, "records are not aligned to their size"); } // (16 / 8 bytes: the kernels store and load a record at once)
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	if (!d_mask || !d_zones) { return fail(ALPGPU_ERR_INVALID, "null bitmap or records"); }
	ALPGPU_TRY(check_n_vectors(col->n_vectors, "column.n_vectors is implausible"));
	ALPGPU_TRY(check_has_descriptors(col));
	const int rc = alpgpu::launch_minmax_masked(ctx->stream, col, d_mask, d_zones, d_counts, value_bytes);
	if (rc != ALPGPU_OK) { return fail(rc, "decode_minmax_masked launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}

// lo, hi: the entry point's host arrays, widened to double (exactly) by the caller
static int group_minmax(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const double* lo, const double* hi, uint32_t n_groups,
                        void* d_zones, uint32_t* d_counts, int value_bytes) {
	if (!val || !key) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (val->n_vectors != key->n_vectors) { return fail(ALPGPU_ERR_INVALID, "the columns differ in n_vectors"); }
	ALPGPU_TRY(check_n_vectors(val->n_vectors, "column.n_vectors is implausible"));
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	if (misaligned(d_zones, 2u * value_bytes)) { return fail(ALPGPU_ERR_INVALID, "records are not aligned to their size"); }
	if (val->n_vectors == 0) { return ALPGPU_OK; }
	if (!d_mask || !d_zones) { return fail(ALPGPU_ERR_INVALID, "null bitmap or records"); }
	ALPGPU_TRY(check_has_descriptors(val, key));
	const int rc = alpgpu::launch_group_minmax(ctx->stream, val, key, d_mask, lo, hi, n_groups, d_zones, d_counts, value_bytes);
	if (rc != ALPGPU_OK) { return fail(rc, "decode_group_minmax launch failed"); }
	return ALPGPU_OK;
}

static int check_groups(const void* lo, const void* hi, uint32_t n_groups) {
	if (!lo || !hi) { return fail(ALPGPU_ERR_INVALID, "null bounds"); }
	if (n_groups == 0 || n_groups > ALPGPU_GROUP_MAX) { return fail(ALPGPU_ERR_INVALID, "n_groups is not in 1 .. ALPGPU_GROUP_MAX"); }
	return ALPGPU_OK;
}

static int group_minmax_totals(alpgpu_ctx* ctx, const void* d_zones, uint64_t n_vectors, uint32_t n_groups, void* d_minmax, int value_bytes) {
	if (n_groups == 0 || n_groups > ALPGPU_GROUP_MAX) { return fail(ALPGPU_ERR_INVALID, "n_groups is not in 1 .. ALPGPU_GROUP_MAX"); }
	if (!d_minmax || (n_vectors > 0 && !d_zones)) { return fail(ALPGPU_ERR_INVALID, "null records or result"); }
	if (misaligned(d_zones, 2u * value_bytes) || misaligned(d_minmax, value_bytes)) { return fail(ALPGPU_ERR_INVALID, "records not aligned to their size or result not to its type"); }
	ALPGPU_TRY(check_n_vectors(n_vectors, "n_vectors is implausible"));
	const int rc = alpgpu::launch_group_minmax_totals(ctx->stream, d_zones, n_vectors, n_groups, d_minmax, value_bytes);
	if (rc != ALPGPU_OK) { return fail(rc, "group_minmax_totals launch failed"); }
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

int alpgpu_decode_minmax_masked_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, alpgpu_zone_f64* d_zones, uint32_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	return minmax_masked(ctx, col, d_mask, d_zones, d_counts, 8);
}
int alpgpu_decode_minmax_masked_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, alpgpu_zone_f32* d_zones, uint32_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	return minmax_masked(ctx, col, d_mask, d_zones, d_counts, 4);
}

int alpgpu_decode_group_minmax_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const double* lo, const double* hi, uint32_t n_groups,
                                   alpgpu_zone_f64* d_zones, uint32_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	const int ok = check_groups(lo, hi, n_groups);
	if (ok != ALPGPU_OK) { return ok; }
	return group_minmax(ctx, val, key, d_mask, lo, hi, n_groups, d_zones, d_counts, 8);
}
int alpgpu_decode_group_minmax_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const float* lo, const float* hi, uint32_t n_groups,
                                   alpgpu_zone_f32* d_zones, uint32_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	const int ok = check_groups(lo, hi, n_groups);
	if (ok != ALPGPU_OK) { return ok; }
	double wlo[ALPGPU_GROUP_MAX], whi[ALPGPU_GROUP_MAX]; // (a float passes through double unchanged, NaN and -0.0 included)
	for (uint32_t g = 0; g < n_groups; ++g) {
		wlo[g] = static_cast<double>(lo[g]);
		whi[g] = static_cast<double>(hi[g]);
	}
	return group_minmax(ctx, val, key, d_mask, wlo, whi, n_groups, d_zones, d_counts, 4);
}

int alpgpu_group_minmax_totals_f64(alpgpu_ctx* ctx, const alpgpu_zone_f64* d_zones, uint64_t n_vectors, uint32_t n_groups, double* d_minmax) {
	ALPGPU_CHECK_CTX(ctx);
	return group_minmax_totals(ctx, d_zones, n_vectors, n_groups, d_minmax, 8);
}
int alpgpu_group_minmax_totals_f32(alpgpu_ctx* ctx, const alpgpu_zone_f32* d_zones, uint64_t n_vectors, uint32_t n_groups, float* d_minmax) {
	ALPGPU_CHECK_CTX(ctx);
	return group_minmax_totals(ctx, d_zones, n_vectors, n_groups, d_minmax, 4);
}

} // extern "C"
