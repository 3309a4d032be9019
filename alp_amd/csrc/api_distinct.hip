// api_distinct.hip — distinct values of include/alpgpu.h: alpgpu_distinct_*, their debug entry points and alpgpu_distinct_scratch_bytes.  A call is the
// launches of distinct_kernels.hip on the context's stream and nothing else: no host synchronisation, no second stream, no allocation, and none of what
// the context remembers about columns is read or written.
#include "host_ctx.hpp"

extern "C++" {
// first, n: checked as by alpgpu_histogram_* (the shared checks of host_ctx.hpp)
static int distinct(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const void* d_zones, uint64_t capacity, void* d_vals,
                    uint64_t* d_counts, uint64_t* d_state, void* d_scratch, int value_bytes, const alpgpu_distinct_tuning* tuning, uint64_t* d_trace) {
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (capacity == 0 || capacity > ALPGPU_DISTINCT_MAX) { return fail(ALPGPU_ERR_INVALID, "capacity is not in 1 .. ALPGPU_DISTINCT_MAX"); }
	if (!d_vals || !d_state || !d_scratch) { return fail(ALPGPU_ERR_INVALID, "null values, state or scratch"); }
	ALPGPU_TRY(check_n_vectors(col->n_vectors, "column.n_vectors is implausible"));
	ALPGPU_TRY(check_value_range(col->n_vectors, first, n, "range reaches past the column's last value"));
	ALPGPU_TRY(check_bitmap_aligned(d_mask));
	if (misaligned(d_scratch, 16u)) { return fail(ALPGPU_ERR_INVALID, "scratch is not 16-byte aligned"); }
	if (misaligned(d_vals, static_cast<unsigned>(value_bytes))) { return fail(ALPGPU_ERR_INVALID, "values are not aligned to their elements"); }
	if (misaligned(d_zones, 2u * value_bytes)) { return fail(ALPGPU_ERR_INVALID, "zones are not aligned to their records"); }
	if (misaligned(d_counts, 8u) || misaligned(d_state, 8u) || misaligned(d_trace, 8u)) { return fail(ALPGPU_ERR_INVALID, "counts, state or trace are not 8-byte aligned"); }
	if (col->n_vectors > 0 && n > 0) { ALPGPU_TRY(check_has_descriptors(col)); }
	if (col->n_vectors == 0 || n == 0) { // nothing is selected: the zero state, and nothing of the column is read
		if (alpgpu::launch_fill_u64(ctx->stream, d_state, 4u, 0ull) != ALPGPU_OK) { return fail(ALPGPU_ERR_HIP, "zeroing the state failed", hipGetLastError()); }
		return ALPGPU_OK;
	}
	const int rc = alpgpu::launch_distinct(ctx->stream, col, first, n, d_mask, d_zones, capacity, d_vals, d_counts, d_state, d_scratch, value_bytes, ctx->n_cus, tuning, d_trace);
	if (rc != ALPGPU_OK) { return fail(rc, "distinct launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

uint64_t alpgpu_distinct_scratch_bytes(uint64_t capacity) {
	alpgpu::DistinctLayout L;
	return alpgpu::distinct_layout(capacity, L) ? L.total : UINT64_MAX;
}

int alpgpu_distinct_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, uint64_t capacity,
                        double* d_vals, uint64_t* d_counts, uint64_t* d_state, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return distinct(ctx, col, first, n, d_mask, d_zones, capacity, d_vals, d_counts, d_state, d_scratch, 8, nullptr, nullptr);
}
int alpgpu_distinct_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, uint64_t capacity,
                        float* d_vals, uint64_t* d_counts, uint64_t* d_state, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return distinct(ctx, col, first, n, d_mask, d_zones, capacity, d_vals, d_counts, d_state, d_scratch, 4, nullptr, nullptr);
}
int alpgpu_debug_distinct_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f64* d_zones, uint64_t capacity,
                              double* d_vals, uint64_t* d_counts, uint64_t* d_state, void* d_scratch, const alpgpu_distinct_tuning* tuning, uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return distinct(ctx, col, first, n, d_mask, d_zones, capacity, d_vals, d_counts, d_state, d_scratch, 8, tuning, d_trace);
}
int alpgpu_debug_distinct_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const alpgpu_zone_f32* d_zones, uint64_t capacity,
                              float* d_vals, uint64_t* d_counts, uint64_t* d_state, void* d_scratch, const alpgpu_distinct_tuning* tuning, uint64_t* d_trace) {
	ALPGPU_CHECK_CTX(ctx);
	return distinct(ctx, col, first, n, d_mask, d_zones, capacity, d_vals, d_counts, d_state, d_scratch, 4, tuning, d_trace);
}

} // extern "C"
