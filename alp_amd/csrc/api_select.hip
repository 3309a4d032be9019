// api_select.hip — selection of include/alpgpu.h: alpgpu_select_range_* (which values of a compressed column lie in [lo, hi], as ascending
// value indices, optionally with the values), alpgpu_select_range_zoned_* (the same with the column's zone map) and the size of their caller-owned scratch.  A call is a handful of launches of select_kernels.hip
// on the context's stream and nothing else: no host synchronisation, no second stream, no allocation, and none of what the context remembers
// about columns (segment tables, learned sizes, the progress word, the read-ahead) is read or written.
#include "host_ctx.hpp"

extern "C++" {
// zoned: the call is alpgpu_select_range_zoned_* and d_zones its zone map (one record of 2 * value_bytes per vector)
static int select_range(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, double lo, double hi, int64_t* d_idx, void* d_vals,
                        uint64_t capacity, uint64_t* d_count, void* d_scratch, int value_bytes, const void* d_zones = nullptr, bool zoned = false) {
	if (!col || !d_count) { return fail(ALPGPU_ERR_INVALID, "null column or count"); }
	ALPGPU_TRY(check_n_vectors(col->n_vectors, "column.n_vectors is implausible"));
	ALPGPU_TRY(check_value_range(col->n_vectors, first, n, "range reaches past the column's last value"));
	if (capacity > 0 && !d_idx) { return fail(ALPGPU_ERR_INVALID, "null index output with a capacity"); }
	if (n == 0) { // nothing can qualify: the count alone is written
		ALPGPU_HIP(hipMemsetAsync(d_count, 0, sizeof(uint64_t), ctx->stream));
		return ALPGPU_OK;
	}
	if (zoned && (!d_zones || misaligned(d_zones, 2u * value_bytes))) { return fail(ALPGPU_ERR_INVALID, "zone map is null or not aligned to its records"); }
	if (!d_scratch || misaligned(d_scratch, 16u)) { return fail(ALPGPU_ERR_INVALID, "scratch is null or not 16-byte aligned"); }
	ALPGPU_TRY(check_has_descriptors(col));
	const int rc = alpgpu::launch_select_range(ctx->stream, col, first, n, lo, hi, d_idx, d_vals, capacity, d_count, d_scratch, value_bytes, zoned ? d_zones : nullptr);
	if (rc != ALPGPU_OK) { return fail(rc, "select launch failed"); } // (the launcher has read the HIP error)
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

uint64_t alpgpu_select_scratch_bytes(uint64_t n_vectors) { return alpgpu::select_scratch_bytes(n_vectors); }

int alpgpu_select_range_f64(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, double lo, double hi, int64_t* d_idx, double* d_vals,
                            uint64_t capacity, uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return select_range(ctx, col, first, n, lo, hi, d_idx, d_vals, capacity, d_count, d_scratch, 8);
}
int alpgpu_select_range_f32(alpgpu_ctx* ctx, const alpgpu_column* col, uint64_t first, uint64_t n, float lo, float hi, int64_t* d_idx, float* d_vals,
                            uint64_t capacity, uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return select_range(ctx, col, first, n, lo, hi, d_idx, d_vals, capacity, d_count, d_scratch, 4);
}

int alpgpu_select_range_zoned_f64(alpgpu_ctx* ctx, const alpgpu_column* col, const alpgpu_zone_f64* d_zones, uint64_t first, uint64_t n, double lo, double hi,
                                  int64_t* d_idx, double* d_vals, uint64_t capacity, uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return select_range(ctx, col, first, n, lo, hi, d_idx, d_vals, capacity, d_count, d_scratch, 8, d_zones, true);
}
int alpgpu_select_range_zoned_f32(alpgpu_ctx* ctx, const alpgpu_column* col, const alpgpu_zone_f32* d_zones, uint64_t first, uint64_t n, float lo, float hi,
                                  int64_t* d_idx, float* d_vals, uint64_t capacity, uint64_t* d_count, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	return select_range(ctx, col, first, n, lo, hi, d_idx, d_vals, capacity, d_count, d_scratch, 4, d_zones, true);
}

int alpgpu_debug_select_scan(alpgpu_ctx* ctx, const uint32_t* d_counts, uint64_t n, uint64_t* d_offsets, uint64_t* d_total, void* d_scratch) {
	ALPGPU_CHECK_CTX(ctx);
	if (n == 0 || n > (1ull << 54) || !d_counts || !d_offsets || !d_total || !d_scratch) { return fail(ALPGPU_ERR_INVALID, "null pointer argument or no counts"); }
	if (alpgpu::launch_select_scan(ctx->stream, d_counts, n, d_offsets, d_total, static_cast<uint64_t*>(d_scratch)) != ALPGPU_OK) {
		return fail(ALPGPU_ERR_HIP, "scan launch failed");
	}
	return ALPGPU_OK;
}

} // extern "C"
