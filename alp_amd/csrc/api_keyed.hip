// api_keyed.hip — keyed aggregation of include/alpgpu.h: alpgpu_decode_keyed_sum_f64, its debug entry point and the two host formulas (double columns
// only: the float entry points are not built, include/alpgpu.h says why).  A call is
// the launches of keyed_kernels.hip on the context's stream and nothing else: no host synchronisation, no second stream, no allocation beyond the
// caller's scratch, and none of what the context remembers about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
static int keyed_sum(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_keys, uint32_t n_keys,
                     double* d_sums, uint64_t* d_counts, void* d_scratch, int value_bytes, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	if (!val || !key) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (!d_keys || !d_sums || !d_scratch) { return fail(ALPGPU_ERR_INVALID, "null keys, sums or scratch"); }
	if (n_keys == 0 || n_keys > ALPGPU_KEYED_KEYS_MAX) { return fail(ALPGPU_ERR_INVALID, "n_keys is not in 1 .. ALPGPU_KEYED_KEYS_MAX"); }
	ALPGPU_TRY(check_pair_n_vectors(val, key));
	if (misaligned(d_scratch, 16u)) { return fail(ALPGPU_ERR_INVALID, "scratch is not 16-byte aligned"); }
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	if (misaligned(d_sums, 8u) || misaligned(d_counts, 8u) || misaligned(d_trace, 8u)) { return fail(ALPGPU_ERR_INVALID, "sums, counts or trace are not 8-byte aligned"); }
	ALPGPU_TRY(check_list_and_zones(d_keys, "keys are not aligned to their elements", d_zones, value_bytes));
	if (val->n_vectors == 0) { // +0.0 and 0 everywhere, by a kernel
		if (alpgpu::launch_fill_u64(ctx->stream, reinterpret_cast<uint64_t*>(d_sums), n_keys, 0ull) != ALPGPU_OK ||
		    (d_counts && alpgpu::launch_fill_u64(ctx->stream, d_counts, n_keys + 1u, 0ull) != ALPGPU_OK)) {
			return fail(ALPGPU_ERR_HIP, "zeroing the sums and counts failed", hipGetLastError());
		}
		return ALPGPU_OK;
	}
	ALPGPU_TRY(check_has_descriptors(val, key));
	const int rc = alpgpu::launch_keyed_sum(ctx->stream, val, key, d_mask, d_zones, d_keys, n_keys, d_sums, d_counts, d_scratch, value_bytes, ctx->n_cus, tuning, d_trace);
	if (rc != ALPGPU_OK) { return fail(rc, "decode_keyed_sum launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

uint64_t alpgpu_keyed_stripe_vectors(uint64_t n_vectors) { return alpgpu::keyed_stripe_vectors(n_vectors); }

uint64_t alpgpu_keyed_sum_scratch_bytes(uint64_t n_vectors, uint32_t n_keys) {
	if (n_keys == 0 || n_keys > ALPGPU_KEYED_KEYS_MAX) { return UINT64_MAX; }
	const uint64_t rows = n_vectors < ALPGPU_KEYED_STRIPES_MAX ? n_vectors : ALPGPU_KEYED_STRIPES_MAX; // >= S = ceil(n_vectors / L), and monotone where S is not
	return (64ull + 8ull * n_keys * rows + 15ull) & ~15ull;
}

int alpgpu_decode_keyed_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones, const double* d_keys,
                                uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return keyed_sum(ctx, val, key, d_mask, d_key_zones, d_keys, n_keys, d_sums, d_counts, d_scratch, 8, nullptr, nullptr);
}
int alpgpu_debug_decode_keyed_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                      const double* d_keys, uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_scratch, const alpgpu_keyed_tuning* tuning,
                                      uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return keyed_sum(ctx, val, key, d_mask, d_key_zones, d_keys, n_keys, d_sums, d_counts, d_scratch, 8, tuning, d_trace);
}

} // extern "C"
