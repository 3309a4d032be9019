// api_in_list.hip — set membership of include/alpgpu.h: alpgpu_select_in_mask_* (`x IN (list)` on a compressed column, set into or combined with a
// caller's bitmap) and alpgpu_in_list_lds_max.  A call is one launch of in_list_kernels.hip on the context's stream and nothing else: no host
// synchronisation, no second stream, no allocation, no atomics on results, and none of what the context remembers about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
// op, first, n: checked, and an empty range settled, as by alpgpu_select_mask_* (the shared checks of host_ctx.hpp)
static int select_in_mask(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const void* d_list, uint64_t n_list, int negate, const void* d_zones, int op,
                          uint64_t* d_mask, int value_bytes) {
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	ALPGPU_TRY(check_mask_op(op));
	ALPGPU_TRY(check_n_vectors(col->n_vectors, "column.n_vectors is implausible"));
	ALPGPU_TRY(check_value_range(col->n_vectors, first, n, "range reaches past the column's last value"));
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	if (n_list > 0x7FFFFFFFull) { return fail(ALPGPU_ERR_INVALID, "n_list is beyond 2^31 - 1"); }
	if (n_list > 0 && !d_list) { return fail(ALPGPU_ERR_INVALID, "null list with n_list > 0"); }
	if (misaligned(d_list, static_cast<unsigned>(value_bytes))) { return fail(ALPGPU_ERR_INVALID, "list is not aligned to its elements"); }
	if (misaligned(d_zones, 2u * value_bytes)) { return fail(ALPGPU_ERR_INVALID, "zones are not aligned to their records"); }
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	if (!d_mask) { return fail(ALPGPU_ERR_INVALID, "null bitmap"); }
	if (n == 0) { return clear_bitmap_for_empty_range(ctx, op, d_mask, col); }
	ALPGPU_TRY(check_has_descriptors(col));
	const int rc = alpgpu::launch_select_in_mask(ctx->stream, col, first, n, d_list, n_list, negate, d_zones, op, d_mask, value_bytes, ctx->n_cus);
	if (rc != ALPGPU_OK) { return fail(rc, "select_in_mask launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

int alpgpu_select_in_mask_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const double* d_list, uint64_t n_list, int negate,
                              const alpgpu_zone_f64* d_zones, int op, uint64_t* d_mask) {
	ALPGPU_CHECK_CTX(ctx);
	return select_in_mask(ctx, col, first, n, d_list, n_list, negate, d_zones, op, d_mask, 8);
}
int alpgpu_select_in_mask_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const float* d_list, uint64_t n_list, int negate,
                              const alpgpu_zone_f32* d_zones, int op, uint64_t* d_mask) {
	ALPGPU_CHECK_CTX(ctx);
	return select_in_mask(ctx, col, first, n, d_list, n_list, negate, d_zones, op, d_mask, 4);
}
size_t alpgpu_in_list_lds_max(int value_bytes) { return alpgpu::in_list_lds_max(value_bytes); }

} // extern "C"
