// api_group.hip — grouped aggregation of include/alpgpu.h: alpgpu_decode_group_sum_* (per-vector SUM and COUNT of a value column for up to
// ALPGPU_GROUP_MAX closed ranges of a key column, under a caller's bitmap) and alpgpu_group_totals (every group's total by the documented tree,
// the counts added up exactly).  A call is launches of group_kernels.hip on the context's stream and nothing else: no host synchronisation, no
// second stream, no allocation, the context's workspace is not used and none of what the context remembers about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
// lo, hi: the entry point's host arrays, widened to double (exactly) by the caller
static int group_sum(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const double* lo, const double* hi, uint32_t n_groups, double* d_sums,
                     uint32_t* d_counts, int value_bytes) {
	if (!val || !key) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (val->n_vectors != key->n_vectors) { return fail(ALPGPU_ERR_INVALID, "the columns differ in n_vectors"); }
	ALPGPU_TRY(check_n_vectors(val->n_vectors, "column.n_vectors is implausible"));
	if (val->n_vectors == 0) { return ALPGPU_OK; }
	if (!d_mask || !d_sums) { return fail(ALPGPU_ERR_INVALID, "null bitmap or sums"); }
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	ALPGPU_TRY(check_has_descriptors(val, key));
	const int rc = alpgpu::launch_group_sum(ctx->stream, val, key, d_mask, lo, hi, n_groups, d_sums, d_counts, value_bytes);
	if (rc != ALPGPU_OK) { return fail(rc, "decode_group_sum launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}

static int check_groups(const void* lo, const void* hi, uint32_t n_groups) {
	if (!lo || !hi) { return fail(ALPGPU_ERR_INVALID, "null bounds"); }
	if (n_groups == 0 || n_groups > ALPGPU_GROUP_MAX) { return fail(ALPGPU_ERR_INVALID, "n_groups is not in 1 .. ALPGPU_GROUP_MAX"); }
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

int alpgpu_decode_group_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const double* lo, const double* hi, uint32_t n_groups,
                                double* d_sums, uint32_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	const int ok = check_groups(lo, hi, n_groups);
	if (ok != ALPGPU_OK) { return ok; }
	return group_sum(ctx, val, key, d_mask, lo, hi, n_groups, d_sums, d_counts, 8);
}
int alpgpu_decode_group_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const float* lo, const float* hi, uint32_t n_groups,
                                double* d_sums, uint32_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	const int ok = check_groups(lo, hi, n_groups);
	if (ok != ALPGPU_OK) { return ok; }
	double wlo[ALPGPU_GROUP_MAX], whi[ALPGPU_GROUP_MAX]; // (a float passes through double unchanged, NaN and -0.0 included)
	for (uint32_t g = 0; g < n_groups; ++g) {
		wlo[g] = static_cast<double>(lo[g]);
		whi[g] = static_cast<double>(hi[g]);
	}
	return group_sum(ctx, val, key, d_mask, wlo, whi, n_groups, d_sums, d_counts, 4);
}

size_t alpgpu_group_totals_scratch_bytes(uint64_t n_vectors, uint32_t n_groups) {
	const uint64_t l1 = (n_vectors + 1023) / 1024;
	return static_cast<size_t>(32ull * l1 * n_groups); // two buffers of sums and two of counts, one 8-byte element per group and block of 1024
}

int alpgpu_group_totals(alpgpu_ctx* ctx, const double* d_sums, const uint32_t* d_counts, uint64_t n_vectors, uint32_t n_groups, double* d_total_sums, uint64_t* d_total_counts,
                        void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	if (n_groups == 0 || n_groups > ALPGPU_GROUP_MAX) { return fail(ALPGPU_ERR_INVALID, "n_groups is not in 1 .. ALPGPU_GROUP_MAX"); }
	if (!d_total_sums) { return fail(ALPGPU_ERR_INVALID, "null totals"); }
	ALPGPU_TRY(check_n_vectors(n_vectors, "n_vectors is implausible"));
	if (n_vectors == 0) { // no row holds anything, so neither input is looked at: an empty array's pointer may well be NULL
		ALPGPU_HIP(hipMemsetAsync(d_total_sums, 0, sizeof(double) * n_groups, ctx->stream));
		if (d_total_counts) { ALPGPU_HIP(hipMemsetAsync(d_total_counts, 0, sizeof(uint64_t) * n_groups, ctx->stream)); }
		return ALPGPU_OK;
	}
	if (!d_sums) { return fail(ALPGPU_ERR_INVALID, "null sums"); }
	if ((d_counts == nullptr) != (d_total_counts == nullptr)) { return fail(ALPGPU_ERR_INVALID, "counts without their totals, or totals without counts"); }
	if (n_vectors > 1024 && (!d_scratch || misaligned(d_scratch, 16u))) { return fail(ALPGPU_ERR_INVALID, "scratch is null or not 16-byte aligned"); }
	const int rc = alpgpu::launch_group_totals(ctx->stream, d_sums, d_counts, n_vectors, n_groups, d_total_sums, d_total_counts, d_scratch);
	if (rc != ALPGPU_OK) { return fail(rc, "group_totals launch failed"); }
	return ALPGPU_OK;
}

} // extern "C"
