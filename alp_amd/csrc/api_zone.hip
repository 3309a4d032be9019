// api_zone.hip — zone maps of include/alpgpu.h: alpgpu_zone_map_* (one {min, max} record per vector of an encoded column, decoded in registers),
// alpgpu_zone_map_of_values_* (the same records from the raw values) and alpgpu_zones_minmax_* (the column's MIN / MAX); the selection that reads
// the records, alpgpu_select_range_zoned_*, is in api_select.hip beside the plain one.  Like gather and select:
// launches on the context's stream and nothing else — no host synchronisation, no allocation, nothing the context remembers about columns.
#include "host_ctx.hpp"

extern "C++" {
// (every misaligned() below: a zone array is aligned to its records, 16 / 8 bytes, because the kernels store and load a record at once, and the raw
// values to the 16 bytes of a load)
static int zone_map(alpgpu_ctx* ctx, const alpgpu_column* col, void* d_zones, int value_bytes) {
	if (!col) { return fail(ALPGPU_ERR_INVALID, "null column"); }
	if (col->n_vectors == 0) { return ALPGPU_OK; }
	if (!d_zones || misaligned(d_zones, 2u * value_bytes)) { return fail(ALPGPU_ERR_INVALID, "zone output is null or not aligned to its records"); }
	ALPGPU_TRY(check_has_descriptors(col));
	const int rc = value_bytes == 8 ? alpgpu::launch_zone_map(ctx->stream, col, d_zones) : alpgpu::launch_zone_map_f32(ctx->stream, col, d_zones);
	if (rc != ALPGPU_OK) { return fail(rc, "zone map launch failed"); }
	return ALPGPU_OK;
}
static int zone_map_of_values(alpgpu_ctx* ctx, const void* d_in, uint64_t n_vectors, void* d_zones, int value_bytes) {
	if (n_vectors == 0) { return ALPGPU_OK; }
	if (!d_in || !d_zones) { return fail(ALPGPU_ERR_INVALID, "null input or zone output"); }
	if (misaligned(d_in, 16u) || misaligned(d_zones, 2u * value_bytes)) { return fail(ALPGPU_ERR_INVALID, "input not 16-byte aligned or zone output not aligned to its records"); }
	if (n_vectors > (~0ull >> 14)) { return fail(ALPGPU_ERR_INVALID, "n_vectors is implausible"); }
	const int rc = alpgpu::launch_zone_map_of_values(ctx->stream, d_in, n_vectors, d_zones, value_bytes);
	if (rc != ALPGPU_OK) { return fail(rc, "zone map launch failed"); }
	return ALPGPU_OK;
}
static int zones_minmax(alpgpu_ctx* ctx, const void* d_zones, uint64_t n_vectors, void* d_minmax, int value_bytes) {
	if (!d_minmax || (n_vectors > 0 && !d_zones)) { return fail(ALPGPU_ERR_INVALID, "null zones or result"); }
	if (misaligned(d_zones, 2u * value_bytes) || misaligned(d_minmax, value_bytes)) { return fail(ALPGPU_ERR_INVALID, "zones not aligned to their records or result not to its type"); }
	if (n_vectors > (~0ull >> 5)) { return fail(ALPGPU_ERR_INVALID, "n_vectors is implausible"); }
	const int rc = alpgpu::launch_zones_minmax(ctx->stream, d_zones, n_vectors, d_minmax, value_bytes);
	if (rc != ALPGPU_OK) { return fail(rc, "zone reduction launch failed"); }
	return ALPGPU_OK;
}
} // extern "C++"

extern "C" {

int alpgpu_zone_map_f64(alpgpu_ctx* ctx, const alpgpu_column* col, alpgpu_zone_f64* d_zones) {
	ALPGPU_CHECK_CTX(ctx);
	return zone_map(ctx, col, d_zones, 8);
}
int alpgpu_zone_map_f32(alpgpu_ctx* ctx, const alpgpu_column* col, alpgpu_zone_f32* d_zones) {
	ALPGPU_CHECK_CTX(ctx);
	return zone_map(ctx, col, d_zones, 4);
}
int alpgpu_zone_map_of_values_f64(alpgpu_ctx* ctx, const double* d_in, uint64_t n_vectors, alpgpu_zone_f64* d_zones) {
	ALPGPU_CHECK_CTX(ctx);
	return zone_map_of_values(ctx, d_in, n_vectors, d_zones, 8);
}
int alpgpu_zone_map_of_values_f32(alpgpu_ctx* ctx, const float* d_in, uint64_t n_vectors, alpgpu_zone_f32* d_zones) {
	ALPGPU_CHECK_CTX(ctx);
	return zone_map_of_values(ctx, d_in, n_vectors, d_zones, 4);
}
int alpgpu_zones_minmax_f64(alpgpu_ctx* ctx, const alpgpu_zone_f64* d_zones, uint64_t n_vectors, double* d_minmax) {
	ALPGPU_CHECK_CTX(ctx);
	return zones_minmax(ctx, d_zones, n_vectors, d_minmax, 8);
}
int alpgpu_zones_minmax_f32(alpgpu_ctx* ctx, const alpgpu_zone_f32* d_zones, uint64_t n_vectors, float* d_minmax) {
	ALPGPU_CHECK_CTX(ctx);
	return zones_minmax(ctx, d_zones, n_vectors, d_minmax, 4);
}

} // extern "C"
