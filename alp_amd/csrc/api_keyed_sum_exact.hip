// api_keyed_sum_exact.hip — the exact keyed SUM of include/alpgpu.h: alpgpu_keyed_exact_sum_table_bytes, alpgpu_decode_keyed_exact_sum_f64 / _f32 and their
// debug entry points.  A call is the kernels of keyed_sum_exact_kernels.hip on the context's stream and nothing else: no host synchronisation, no second
// stream, no allocation, and none of what the context remembers about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
static int keyed_sum_exact(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_keys, uint32_t n_keys,
                           double* d_sums, uint64_t* d_counts, void* d_table, int accumulate, int value_bytes, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	if (!val || !key) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (!d_keys || !d_sums || !d_table) { return fail(ALPGPU_ERR_INVALID, "null keys, sums or table"); }
	if (n_keys == 0 || n_keys > ALPGPU_KEYED_MANY_KEYS_MAX) { return fail(ALPGPU_ERR_INVALID, "n_keys is not in 1 .. ALPGPU_KEYED_MANY_KEYS_MAX"); }
	ALPGPU_TRY(check_pair_n_vectors(val, key));
	if (val->n_vectors > ALPGPU_KEYED_EXACT_VECTORS_MAX) { return fail(ALPGPU_ERR_INVALID, "column.n_vectors is beyond ALPGPU_KEYED_EXACT_VECTORS_MAX"); }
	ALPGPU_TRY(check_bitmap_counts_trace(d_mask, d_counts, d_trace));
	if (misaligned(d_sums, 8u)) { return fail(ALPGPU_ERR_INVALID, "the sums are not 8-byte aligned"); }
	if (misaligned(d_table, 16u)) { return fail(ALPGPU_ERR_INVALID, "the table is not 16-byte aligned"); }
	ALPGPU_TRY(check_list_and_zones(d_keys, "keys are not aligned to their elements", d_zones, value_bytes));
	if (val->n_vectors > 0) { ALPGPU_TRY(check_has_descriptors(val, key)); }
	const int rc = alpgpu::launch_keyed_sum_exact(ctx->stream, val, key, d_mask, d_zones, d_keys, n_keys, d_sums, d_counts, d_table, accumulate, value_bytes, ctx->n_cus, tuning, d_trace);
	if (rc != ALPGPU_OK) { return fail(rc, "decode_keyed_exact_sum launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

uint64_t alpgpu_keyed_exact_sum_table_bytes(uint32_t n_keys) {
	return n_keys == 0 || n_keys > ALPGPU_KEYED_MANY_KEYS_MAX ? UINT64_MAX : alpgpu::keyed_sum_exact_table_bytes(n_keys);
}

int alpgpu_decode_keyed_exact_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                      const double* d_keys, uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_table, int accumulate) {
	ALPGPU_CHECK_CTX(ctx);
	return keyed_sum_exact(ctx, val, key, d_mask, d_key_zones, d_keys, n_keys, d_sums, d_counts, d_table, accumulate, 8, nullptr, nullptr);
}
int alpgpu_decode_keyed_exact_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                      const float* d_keys, uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_table, int accumulate) {
	ALPGPU_CHECK_CTX(ctx);
	return keyed_sum_exact(ctx, val, key, d_mask, d_key_zones, d_keys, n_keys, d_sums, d_counts, d_table, accumulate, 4, nullptr, nullptr);
}
int alpgpu_debug_decode_keyed_exact_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                            const double* d_keys, uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_table, int accumulate,
                                            const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return keyed_sum_exact(ctx, val, key, d_mask, d_key_zones, d_keys, n_keys, d_sums, d_counts, d_table, accumulate, 8, tuning, d_trace);
}
int alpgpu_debug_decode_keyed_exact_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                            const float* d_keys, uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_table, int accumulate,
                                            const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return keyed_sum_exact(ctx, val, key, d_mask, d_key_zones, d_keys, n_keys, d_sums, d_counts, d_table, accumulate, 4, tuning, d_trace);
}

} // extern "C"
