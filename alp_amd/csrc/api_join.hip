// api_join.hip — join probe of include/alpgpu.h: alpgpu_join_probe_* (every selected value of a compressed column matched against a sorted key list,
// compacted in index order).  A call is, with a bitmap, the popcount pass and the scan of mask_kernels.hip and then one launch of join_kernels.hip, without
// one that launch alone, on the context's stream and nothing else: no host synchronisation, no second stream, no allocation, no atomics at all, and none
// of what the context remembers about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
static int join_probe(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const void* d_zones, const void* d_keys, uint64_t n_keys, const int64_t* d_rows,
                      int64_t* d_pos, uint32_t* d_span, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch, int value_bytes) {
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (!d_count) { return fail(ALPGPU_ERR_INVALID, "null count"); }
	if (capacity > 0 && !d_pos) { return fail(ALPGPU_ERR_INVALID, "null position output with a capacity"); }
	ALPGPU_TRY(check_n_vectors(col->n_vectors, "column.n_vectors is implausible"));
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	if (n_keys > 0x7FFFFFFFull) { return fail(ALPGPU_ERR_INVALID, "n_keys is beyond 2^31 - 1"); }
	if (n_keys > 0 && !d_keys) { return fail(ALPGPU_ERR_INVALID, "null keys with n_keys > 0"); }
	if (misaligned(d_keys, static_cast<unsigned>(value_bytes))) { return fail(ALPGPU_ERR_INVALID, "keys are not aligned to their elements"); }
	if (misaligned(d_zones, 2u * value_bytes)) { return fail(ALPGPU_ERR_INVALID, "zones are not aligned to their records"); }
	if (misaligned(d_rows, 8u)) { return fail(ALPGPU_ERR_INVALID, "rows are not 8-byte aligned"); }
	if (misaligned(d_count, 8u) || misaligned(d_pos, 8u) || misaligned(d_idx, 8u) || misaligned(d_span, 4u)) { return fail(ALPGPU_ERR_INVALID, "an output is not aligned to its elements"); }
	if (d_mask && col->n_vectors > 0 && (!d_scratch || misaligned(d_scratch, 16u))) { return fail(ALPGPU_ERR_INVALID, "scratch is null or not 16-byte aligned"); }
	if (col->n_vectors == 0) { // no index at all: the count alone is written
		if (alpgpu::launch_fill_u64(ctx->stream, d_count, 1u, 0ull) != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "writing the count failed", hipGetLastError()); }
		return ALPGPU_OK;
	}
	if (capacity > 0) { ALPGPU_TRY(check_has_descriptors(col)); }
	const int rc = alpgpu::launch_join_probe(ctx->stream, col, d_mask, d_zones, d_keys, n_keys, d_rows, d_pos, d_span, d_idx, capacity, d_count, d_scratch, value_bytes, ctx->n_cus);
	if (rc != ALPGPU_OK) { return fail(rc, "join_probe launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

int alpgpu_join_probe_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, const double* d_keys, uint64_t n_keys,
                          const int64_t* d_rows, int64_t* d_pos, uint32_t* d_span, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return join_probe(ctx, col, d_mask, d_zones, d_keys, n_keys, d_rows, d_pos, d_span, d_idx, capacity, d_count, d_scratch, 8);
}
int alpgpu_join_probe_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, const float* d_keys, uint64_t n_keys,
                          const int64_t* d_rows, int64_t* d_pos, uint32_t* d_span, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return join_probe(ctx, col, d_mask, d_zones, d_keys, n_keys, d_rows, d_pos, d_span, d_idx, capacity, d_count, d_scratch, 4);
}

} // extern "C"
