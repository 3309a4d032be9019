// api_bucket.hip — bucketed aggregation of include/alpgpu.h: alpgpu_decode_bucket_sum_f64 / _f32, alpgpu_decode_bucket_minmax_f64 / _f32, their debug
// entry points and the scratch formula.  A call is the launches of bucket_kernels.hip on the context's stream and nothing else: no host
// synchronisation, no second stream, no allocation beyond the caller's scratch, and none of what the context remembers about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
// what both families check alike; d_result: d_sums or d_out
static int bucket_common(const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_edges, uint32_t n_edges,
                         const void* d_result, const uint64_t* d_counts, int value_bytes, const uint64_t* d_trace) {
	if (!val || !key) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (!d_result) { return fail(ALPGPU_ERR_INVALID, "null sums or records"); }
	if (n_edges > ALPGPU_BUCKET_EDGES_MAX) { return fail(ALPGPU_ERR_INVALID, "n_edges is beyond ALPGPU_BUCKET_EDGES_MAX"); }
	if (!d_edges && n_edges > 0) { return fail(ALPGPU_ERR_INVALID, "null edges with n_edges > 0"); }
	ALPGPU_TRY(check_pair_n_vectors(val, key));
	ALPGPU_TRY(check_bitmap_counts_trace(d_mask, d_counts, d_trace));
	return check_list_and_zones(d_edges, "edges are not aligned to their elements", d_zones, value_bytes);
}

static int bucket_sum(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_edges, uint32_t n_edges,
                      int right, double* d_sums, uint64_t* d_counts, void* d_scratch, int value_bytes, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	ALPGPU_TRY(bucket_common(val, key, d_mask, d_zones, d_edges, n_edges, d_sums, d_counts, value_bytes, d_trace));
	if (!d_scratch) { return fail(ALPGPU_ERR_INVALID, "null scratch"); }
	if (misaligned(d_scratch, 16u)) { return fail(ALPGPU_ERR_INVALID, "scratch is not 16-byte aligned"); }
	if (misaligned(d_sums, 8u)) { return fail(ALPGPU_ERR_INVALID, "sums are not 8-byte aligned"); }
	if (val->n_vectors == 0) { // +0.0 and 0 everywhere, by a kernel
		if (alpgpu::launch_fill_u64(ctx->stream, reinterpret_cast<uint64_t*>(d_sums), n_edges + 1u, 0ull) != ALPGPU_OK ||
		    (d_counts && alpgpu::launch_fill_u64(ctx->stream, d_counts, n_edges + 2u, 0ull) != ALPGPU_OK)) {
			return fail(ALPGPU_ERR_HIP, "zeroing the sums and counts failed", hipGetLastError());
		}
		return ALPGPU_OK;
	}
	ALPGPU_TRY(check_has_descriptors(val, key));
	const int rc = alpgpu::launch_bucket_sum(ctx->stream, val, key, d_mask, d_zones, d_edges, n_edges, right, d_sums, d_counts, d_scratch, value_bytes, ctx->n_cus, tuning, d_trace);
	if (rc != ALPGPU_OK) { return fail(rc, "decode_bucket_sum launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}

static int bucket_minmax(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_edges, uint32_t n_edges,
                         int right, void* d_out, uint64_t* d_counts, int value_bytes, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	ALPGPU_TRY(bucket_common(val, key, d_mask, d_zones, d_edges, n_edges, d_out, d_counts, value_bytes, d_trace));
	if (misaligned(d_out, 2u * value_bytes)) { return fail(ALPGPU_ERR_INVALID, "the records are not aligned to their size"); }
	bool done;
	ALPGPU_TRY(minmax_empty_or_descriptors(ctx, val, key, d_out, d_counts, n_edges + 1u, value_bytes, &done));
	if (done) { return ALPGPU_OK; }
	const int rc = alpgpu::launch_bucket_minmax(ctx->stream, val, key, d_mask, d_zones, d_edges, n_edges, right, d_out, d_counts, value_bytes, ctx->n_cus, tuning, d_trace);
	if (rc != ALPGPU_OK) { return fail(rc, "decode_bucket_minmax launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

uint64_t alpgpu_bucket_sum_scratch_bytes(uint64_t n_vectors, uint32_t n_edges) {
	if (n_edges > ALPGPU_BUCKET_EDGES_MAX) { return UINT64_MAX; }
	return alpgpu_keyed_sum_scratch_bytes(n_vectors, n_edges + 1u);
}

int alpgpu_decode_bucket_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                 const double* d_edges, uint32_t n_edges, int right, double* d_sums, uint64_t* d_counts, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return bucket_sum(ctx, val, key, d_mask, d_key_zones, d_edges, n_edges, right, d_sums, d_counts, d_scratch, 8, nullptr, nullptr);
}
int alpgpu_decode_bucket_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                 const float* d_edges, uint32_t n_edges, int right, double* d_sums, uint64_t* d_counts, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return bucket_sum(ctx, val, key, d_mask, d_key_zones, d_edges, n_edges, right, d_sums, d_counts, d_scratch, 4, nullptr, nullptr);
}
int alpgpu_decode_bucket_minmax_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                    const double* d_edges, uint32_t n_edges, int right, alpgpu_zone_f64* d_out, uint64_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	return bucket_minmax(ctx, val, key, d_mask, d_key_zones, d_edges, n_edges, right, d_out, d_counts, 8, nullptr, nullptr);
}
int alpgpu_decode_bucket_minmax_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                    const float* d_edges, uint32_t n_edges, int right, alpgpu_zone_f32* d_out, uint64_t* d_counts) {
	ALPGPU_CHECK_CTX(ctx);
	return bucket_minmax(ctx, val, key, d_mask, d_key_zones, d_edges, n_edges, right, d_out, d_counts, 4, nullptr, nullptr);
}
int alpgpu_debug_decode_bucket_sum_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                       const double* d_edges, uint32_t n_edges, int right, double* d_sums, uint64_t* d_counts, void* d_scratch,
                                       const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return bucket_sum(ctx, val, key, d_mask, d_key_zones, d_edges, n_edges, right, d_sums, d_counts, d_scratch, 8, tuning, d_trace);
}
int alpgpu_debug_decode_bucket_sum_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                       const float* d_edges, uint32_t n_edges, int right, double* d_sums, uint64_t* d_counts, void* d_scratch,
                                       const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return bucket_sum(ctx, val, key, d_mask, d_key_zones, d_edges, n_edges, right, d_sums, d_counts, d_scratch, 4, tuning, d_trace);
}
int alpgpu_debug_decode_bucket_minmax_f64(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f64* d_key_zones,
                                          const double* d_edges, uint32_t n_edges, int right, alpgpu_zone_f64* d_out, uint64_t* d_counts,
                                          const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return bucket_minmax(ctx, val, key, d_mask, d_key_zones, d_edges, n_edges, right, d_out, d_counts, 8, tuning, d_trace);
}
int alpgpu_debug_decode_bucket_minmax_f32(alpgpu_ctx* ctx, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const alpgpu_zone_f32* d_key_zones,
                                          const float* d_edges, uint32_t n_edges, int right, alpgpu_zone_f32* d_out, uint64_t* d_counts,
                                          const alpgpu_keyed_tuning* tuning, uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return bucket_minmax(ctx, val, key, d_mask, d_key_zones, d_edges, n_edges, right, d_out, d_counts, 4, tuning, d_trace);
}

} // extern "C"
