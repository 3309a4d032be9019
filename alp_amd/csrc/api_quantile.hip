// api_quantile.hip — quantiles of include/alpgpu.h: alpgpu_quantile_scratch_bytes, alpgpu_select_rank_*, alpgpu_quantile_* and their debug entry
// points.  A call is one memset and launches of quantile_kernels.hip on the context's stream and nothing else: no host synchronisation (but in
// alpgpu_debug_quantile_trace), no second stream, no allocation, the context's workspace is not used and none of what the context remembers about
// columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
// q != nullptr: the quantile form (n quantiles, d_ranks nullable), else the rank form (n ranks)
static int quantile(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const void* d_zones, const double* q, const uint64_t* ranks, bool quantile_form, uint32_t n,
                    int from_top, void* d_vals, uint64_t* d_ranks, uint64_t* d_count, void* d_scratch, int value_bytes, const alpgpu_quantile_tuning* tuning) {
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (!d_count || !d_vals || !d_mask || !d_scratch) { return fail(ALPGPU_ERR_INVALID, "null count, values, bitmap or scratch"); }
	if (quantile_form ? !q : !ranks) { return fail(ALPGPU_ERR_INVALID, quantile_form ? "null q" : "null ranks"); }
	if (n == 0 || n > (quantile_form ? ALPGPU_QUANTILE_MAX : ALPGPU_RANK_MAX)) {
		return fail(ALPGPU_ERR_INVALID, quantile_form ? "n_q is 0 or more than ALPGPU_QUANTILE_MAX" : "n_ranks is 0 or more than ALPGPU_RANK_MAX");
	}
	if (quantile_form) {
		for (uint32_t i = 0; i < n; ++i) {
			if (!(q[i] >= 0.0 && q[i] <= 1.0)) { return fail(ALPGPU_ERR_INVALID, "a quantile lies outside [0, 1] or is a NaN"); }
		}
	}
	if (misaligned(d_mask, 8u) || misaligned(d_count, 8u) || misaligned(d_ranks, 8u)) { return fail(ALPGPU_ERR_INVALID, "bitmap, count or ranks are not 8-byte aligned"); }
	if (misaligned(d_vals, value_bytes)) { return fail(ALPGPU_ERR_INVALID, "values are not aligned to their type"); }
	if (misaligned(d_zones, 2u * value_bytes) || misaligned(d_scratch, 16u)) { return fail(ALPGPU_ERR_INVALID, "zones are not aligned to their records or the scratch is not 16-byte aligned"); }
	if (col->n_vectors > 0xFFFFFFFFull) { return fail(ALPGPU_ERR_INVALID, "column.n_vectors is implausible"); }
	if (col->n_vectors > 0) { ALPGPU_TRY(check_has_descriptors(col)); }
	if (col->n_vectors == 0) { // nothing is selected: the count alone is written
		ALPGPU_HIP(hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
		return ALPGPU_OK;
	}
	const int rc = alpgpu::launch_quantile(ctx->stream, col, d_mask, d_zones, quantile_form ? q : nullptr, ranks, n, from_top, d_vals, d_ranks, d_count, d_scratch, value_bytes,
	                                       ctx->n_cus, tuning);
	if (rc != ALPGPU_OK) { return fail(rc, "quantile launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

uint64_t alpgpu_quantile_scratch_bytes(uint64_t n_vectors) {
	alpgpu::QuantileLayout L;
	return alpgpu::quantile_layout(n_vectors, L) ? L.total : UINT64_MAX;
}

int alpgpu_select_rank_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, const uint64_t* ranks, uint32_t n_ranks, int from_top,
                           double* d_vals, uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return quantile(ctx, col, d_mask, d_zones, nullptr, ranks, false, n_ranks, from_top, d_vals, nullptr, d_count, d_scratch, 8, nullptr);
}
int alpgpu_select_rank_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, const uint64_t* ranks, uint32_t n_ranks, int from_top,
                           float* d_vals, uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return quantile(ctx, col, d_mask, d_zones, nullptr, ranks, false, n_ranks, from_top, d_vals, nullptr, d_count, d_scratch, 4, nullptr);
}
int alpgpu_quantile_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, const double* q, uint32_t n_q, double* d_vals,
                        uint64_t* d_ranks, uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return quantile(ctx, col, d_mask, d_zones, q, nullptr, true, n_q, 0, d_vals, d_ranks, d_count, d_scratch, 8, nullptr);
}
int alpgpu_quantile_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, const double* q, uint32_t n_q, float* d_vals,
                        uint64_t* d_ranks, uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return quantile(ctx, col, d_mask, d_zones, q, nullptr, true, n_q, 0, d_vals, d_ranks, d_count, d_scratch, 4, nullptr);
}

int alpgpu_debug_quantile_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, const uint64_t* ranks, uint32_t n_ranks,
                              int from_top, double* d_vals, uint64_t* d_count, void* d_scratch, const alpgpu_quantile_tuning* tuning) {
	ALPGPU_CHECK_CTX(ctx);
	return quantile(ctx, col, d_mask, d_zones, nullptr, ranks, false, n_ranks, from_top, d_vals, nullptr, d_count, d_scratch, 8, tuning);
}
int alpgpu_debug_quantile_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, const uint64_t* ranks, uint32_t n_ranks,
                              int from_top, float* d_vals, uint64_t* d_count, void* d_scratch, const alpgpu_quantile_tuning* tuning) {
	ALPGPU_CHECK_CTX(ctx);
	return quantile(ctx, col, d_mask, d_zones, nullptr, ranks, false, n_ranks, from_top, d_vals, nullptr, d_count, d_scratch, 4, tuning);
}
int alpgpu_debug_quantile_trace(alpgpu_ctx* ctx, const void* d_scratch, alpgpu_quantile_trace* out) {
	ALPGPU_CHECK_CTX(ctx);
	if (!d_scratch || !out) { return fail(ALPGPU_ERR_INVALID, "null scratch or trace"); }
	if (alpgpu::quantile_trace(ctx->stream, d_scratch, out) != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "reading the trace failed", hipGetLastError()); }
	return ALPGPU_OK;
}

} // extern "C"
