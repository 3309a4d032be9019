// api_top_k.hip — top-k of include/alpgpu.h: alpgpu_top_k_scratch_bytes and alpgpu_top_k_* (ORDER BY x [DESC] LIMIT k over a compressed column under a
// selection bitmap).  A call is one memset and launches of top_k_kernels.hip (and, without records, of minmax_kernels.hip) on the context's stream and
// nothing else: no host synchronisation, no second stream, no allocation, the context's workspace is not used and none of what the context remembers
// about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
static int top_k(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const void* d_records, uint64_t k, int largest, void* d_vals, int64_t* d_idx, uint64_t* d_count,
                 void* d_scratch, int value_bytes) {
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (!d_count || !d_vals || !d_mask || !d_scratch) { return fail(ALPGPU_ERR_INVALID, "null count, values, bitmap or scratch"); }
	if (k > ALPGPU_TOP_K_MAX) { return fail(ALPGPU_ERR_INVALID, "k is more than ALPGPU_TOP_K_MAX"); }
	if (misaligned(d_mask, 8u) || misaligned(d_count, 8u)) { return fail(ALPGPU_ERR_INVALID, "bitmap or count is not 8-byte aligned"); }
	if (misaligned(d_vals, value_bytes) || misaligned(d_idx, 8u)) { return fail(ALPGPU_ERR_INVALID, "values or indices are not aligned to their type"); }
	if (misaligned(d_records, 16u) || misaligned(d_scratch, 16u)) { return fail(ALPGPU_ERR_INVALID, "records or scratch are not 16-byte aligned"); }
	if (col->n_vectors > 0xFFFFFFFFull) { return fail(ALPGPU_ERR_INVALID, "column.n_vectors is implausible"); }
	if (col->n_vectors > 0) { ALPGPU_TRY(check_has_descriptors(col)); }
	if (k == 0 || col->n_vectors == 0) { // nothing to select: the count alone is written
		ALPGPU_HIP(hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
		return ALPGPU_OK;
	}
	const int rc = alpgpu::launch_top_k(ctx->stream, col, d_mask, d_records, static_cast<uint32_t>(k), largest, d_vals, d_idx, d_count, d_scratch, value_bytes);
	if (rc != ALPGPU_OK) { return fail(rc, "top_k launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

uint64_t alpgpu_top_k_scratch_bytes(uint64_t n_vectors, uint64_t k) {
	alpgpu::TopKLayout L;
	return alpgpu::top_k_layout(n_vectors, k, L) ? L.total : UINT64_MAX;
}

int alpgpu_top_k_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f64* d_records, uint64_t k, int largest, double* d_vals, int64_t* d_idx,
                     uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return top_k(ctx, col, d_mask, d_records, k, largest, d_vals, d_idx, d_count, d_scratch, 8);
}
int alpgpu_top_k_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f32* d_records, uint64_t k, int largest, float* d_vals, int64_t* d_idx,
                     uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return top_k(ctx, col, d_mask, d_records, k, largest, d_vals, d_idx, d_count, d_scratch, 4);
}

} // extern "C"
