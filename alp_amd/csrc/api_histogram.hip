// api_histogram.hip — histograms of include/alpgpu.h: alpgpu_histogram_* and their debug entry points.  A call is the zeroing of its counts (unless it
// accumulates) and one launch of histogram_kernels.hip on the context's stream and nothing else: no host synchronisation, no second stream, no allocation, no
// scratch, and none of what the context remembers about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
// first, n: checked as by alpgpu_select_in_mask_* (the shared checks of host_ctx.hpp)
static int histogram(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const void* d_zones, const void* d_edges, uint32_t n_edges,
                     int right, int accumulate, uint64_t* d_counts, int value_bytes, const alpgpu_histogram_tuning* tuning, uint64_t* d_trace) {
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	ALPGPU_TRY(check_n_vectors(col->n_vectors, "column.n_vectors is implausible"));
	ALPGPU_TRY(check_value_range(col->n_vectors, first, n, "range reaches past the column's last value"));
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	if (n_edges > ALPGPU_HISTOGRAM_EDGES_MAX) { return fail(ALPGPU_ERR_INVALID, "n_edges is beyond ALPGPU_HISTOGRAM_EDGES_MAX"); }
	if (n_edges > 0 && !d_edges) { return fail(ALPGPU_ERR_INVALID, "null edges with n_edges > 0"); }
	if (misaligned(d_edges, static_cast<unsigned>(value_bytes))) { return fail(ALPGPU_ERR_INVALID, "edges are not aligned to their elements"); }
	if (misaligned(d_zones, 2u * value_bytes)) { return fail(ALPGPU_ERR_INVALID, "zones are not aligned to their records"); }
	if (!d_counts) { return fail(ALPGPU_ERR_INVALID, "null counts"); }
	if (misaligned(d_counts, 8u) || misaligned(d_trace, 8u)) { return fail(ALPGPU_ERR_INVALID, "counts or trace are not 8-byte aligned"); }
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	if (n > 0) { ALPGPU_TRY(check_has_descriptors(col)); }
	if (!accumulate && alpgpu::launch_fill_u64(ctx->stream, d_counts, n_edges + 2u, 0ull) != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "zeroing the counts failed", hipGetLastError()); }
	if (n == 0) { return ALPGPU_OK; }
	const int rc = alpgpu::launch_histogram(ctx->stream, col, first, n, d_mask, d_zones, d_edges, n_edges, right, d_counts, value_bytes, ctx->n_cus, tuning, d_trace);
	if (rc != ALPGPU_OK) { return fail(rc, "histogram launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

int alpgpu_histogram_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, const double* d_edges,
                         uint32_t n_edges, int right, int accumulate, uint64_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	return histogram(ctx, col, first, n, d_mask, d_zones, d_edges, n_edges, right, accumulate, d_counts, 8, nullptr, nullptr);
}
int alpgpu_histogram_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, const float* d_edges,
                         uint32_t n_edges, int right, int accumulate, uint64_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	return histogram(ctx, col, first, n, d_mask, d_zones, d_edges, n_edges, right, accumulate, d_counts, 4, nullptr, nullptr);
}
int alpgpu_debug_histogram_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, const double* d_edges,
                               uint32_t n_edges, int right, int accumulate, uint64_t* d_counts, const alpgpu_histogram_tuning* tuning, uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return histogram(ctx, col, first, n, d_mask, d_zones, d_edges, n_edges, right, accumulate, d_counts, 8, tuning, d_trace);
}
int alpgpu_debug_histogram_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, const float* d_edges,
                               uint32_t n_edges, int right, int accumulate, uint64_t* d_counts, const alpgpu_histogram_tuning* tuning, uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return histogram(ctx, col, first, n, d_mask, d_zones, d_edges, n_edges, right, accumulate, d_counts, 4, tuning, d_trace);
}

} // extern "C"
