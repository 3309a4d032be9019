// api_keyed_minmax_many.hip — keyed MIN / MAX for up to 2^20 keys of include/alpgpu.h: alpgpu_decode_keyed_minmax_many_f64 / _f32 and their debug entry
// points.  A call is the init kernel of keyed_minmax_kernels.hip and the one launch of keyed_minmax_many_kernels.hip on the context's stream and nothing
// else: no host synchronisation, no second stream, no allocation, no scratch, and none of what the context remembers about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
static int keyed_minmax_many(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_keys, uint32_t n_keys,
                             void* d_out, uint64_t* d_counts, int value_bytes, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	if (!val || !key) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (!d_keys || !d_out) { return fail(ALPGPU_ERR_INVALID, "null keys or records"); }
	if (n_keys == 0 || n_keys > ALPGPU_KEYED_MANY_KEYS_MAX) { return fail(ALPGPU_ERR_INVALID, "n_keys is not in 1 .. ALPGPU_KEYED_MANY_KEYS_MAX"); }
	ALPGPU_TRY(check_pair_n_vectors(val, key));
	ALPGPU_TRY(check_bitmap_counts_trace(d_mask, d_counts, d_trace));
	if (misaligned(d_out, 2u * value_bytes)) { return fail(ALPGPU_ERR_INVALID, "the records are not aligned to their size"); }
	ALPGPU_TRY(check_list_and_zones(d_keys, "keys are not aligned to their elements", d_zones, value_bytes));
	bool done;
	ALPGPU_TRY(minmax_empty_or_descriptors(ctx, val, key, d_out, d_counts, n_keys, value_bytes, &done));
	if (done) { return ALPGPU_OK; }
	const int rc = alpgpu::launch_keyed_minmax_many(ctx->stream, val, key, d_mask, d_zones, d_keys, n_keys, d_out, d_counts, value_bytes, ctx->n_cus, tuning, d_trace);
	if (rc != ALPGPU_OK) { return fail(rc, "decode_keyed_minmax_many launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

int alpgpu_decode_keyed_minmax_many_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                        const double* d_keys, uint32_t n_keys, alpgpu_zone_f64* d_out, uint64_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	return keyed_minmax_many(ctx, val, key, d_mask, d_key_zones, d_keys, n_keys, d_out, d_counts, 8, nullptr, nullptr);
}
int alpgpu_decode_keyed_minmax_many_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                        const float* d_keys, uint32_t n_keys, alpgpu_zone_f32* d_out, uint64_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	return keyed_minmax_many(ctx, val, key, d_mask, d_key_zones, d_keys, n_keys, d_out, d_counts, 4, nullptr, nullptr);
}
int alpgpu_debug_decode_keyed_minmax_many_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                              const double* d_keys, uint32_t n_keys, alpgpu_zone_f64* d_out, uint64_t* d_counts, const alpgpu_keyed_tuning* tuning,
                                              uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return keyed_minmax_many(ctx, val, key, d_mask, d_key_zones, d_keys, n_keys, d_out, d_counts, 8, tuning, d_trace);
}
int alpgpu_debug_decode_keyed_minmax_many_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                              const float* d_keys, uint32_t n_keys, alpgpu_zone_f32* d_out, uint64_t* d_counts, const alpgpu_keyed_tuning* tuning,
                                              uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return keyed_minmax_many(ctx, val, key, d_mask, d_key_zones, d_keys, n_keys, d_out, d_counts, 4, tuning, d_trace);
}

} // extern "C"
