// api_gather.hip — random access of include/alpgpu.h: alpgpu_gather_* (values by index) and alpgpu_decode_slice_* (a run of values from any index on).
// Both are one launch of gather_kernels.hip on the context's stream and nothing else: no host synchronisation, and none of what the context
// remembers about columns (segment tables, learned sizes, the progress word, the read-ahead) is read or written.
#include "host_ctx.hpp"

extern "C++" {
// the column's value count, n_vectors * 1024 (false: it does not fit in 64 bits)
static bool column_values(const alpgpu_column* col, uint64_t* n_values) {
	if (col->n_vectors > (~0ull >> 10)) { return false; }
	*n_values = col->n_vectors << 10;
	return true;
}

static int gather(alpgpu_ctx* ctx, const alpgpu_column* col, const int64_t* d_idx, uint64_t n, void* d_out, int value_bytes) {
	if (n == 0) { return ALPGPU_OK; }
	if (!col || !d_idx || !d_out) { return fail(ALPGPU_ERR_INVALID, "null column, index or output"); }
	uint64_t n_values = 0;
	if (!column_values(col, &n_values)) { return fail(ALPGPU_ERR_INVALID, "column.n_vectors is implausible"); }
	if (n_values != 0 && (!col->d_vectors || !col->d_rowgroups)) { return fail(ALPGPU_ERR_INVALID, "column has no descriptors"); }
	if (alpgpu::launch_gather(ctx->stream, col, d_idx, 0, n, d_out, value_bytes) != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "gather launch failed", hipGetLastError()); }
	return ALPGPU_OK;
}

static int decode_slice(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, void* d_out, int value_bytes) {
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	uint64_t n_values = 0;
	if (!column_values(col, &n_values)) { return fail(ALPGPU_ERR_INVALID, "column.n_vectors is implausible"); }
	if (first > n_values || n > n_values - first) { return fail(ALPGPU_ERR_INVALID, "slice reaches past the column's last value"); } // (first + n without the overflow)
	if (n == 0) { return ALPGPU_OK; }
	if (!d_out) { return fail(ALPGPU_ERR_INVALID, "null output"); }
	if (!col->d_vectors || !col->d_rowgroups) { return fail(ALPGPU_ERR_INVALID, "column has no descriptors"); }
	if (alpgpu::launch_gather(ctx->stream, col, nullptr, first, n, d_out, value_bytes) != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "slice launch failed", hipGetLastError()); }
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

int alpgpu_gather_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const int64_t* d_idx, uint64_t n, double* d_out) {
	ALPGPU_CHECK_CTX(ctx);
	return gather(ctx, col, d_idx, n, d_out, 8);
}
int alpgpu_gather_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const int64_t* d_idx, uint64_t n, float* d_out) {
	ALPGPU_CHECK_CTX(ctx);
	return gather(ctx, col, d_idx, n, d_out, 4);
}
int alpgpu_decode_slice_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, double* d_out) {
	ALPGPU_CHECK_CTX(ctx);
	return decode_slice(ctx, col, first, n, d_out, 8);
}
int alpgpu_decode_slice_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, float* d_out) {
	ALPGPU_CHECK_CTX(ctx);
	return decode_slice(ctx, col, first, n, d_out, 4);
}

} // extern "C"
