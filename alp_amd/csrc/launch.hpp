// launch.hpp — host-side launch functions implemented by the *.hip kernel files (internal to libalpgpu.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/alpgpu.h"
#include "decode_policy.hpp"
#include "persistent_launch.hpp"

namespace alpgpu {

// A grid dimension holds < 2^31 workgroups: a launch over n_wg workgroups goes out in chunks of at most 2^30, and launch(grid, first workgroup of the chunk) makes
// each — the kernels take that offset as an argument.
inline uint64_t grid_chunk(uint64_t n_wg_left) { constexpr uint64_t kMaxGrid = 1ull << 30; return n_wg_left < kMaxGrid ? n_wg_left : kMaxGrid; }
template <class Launch> inline void launch_in_grid_chunks(uint64_t n_wg, Launch&& launch) {
	for (uint64_t off = 0; off < n_wg; off += grid_chunk(n_wg - off)) { launch(dim3(static_cast<unsigned>(grid_chunk(n_wg - off))), off); }
}

// A kernel over a column's vectors, n_wg workgroups in all: kernel(the column's four streams, out, n_vectors, first workgroup of the chunk, rest...)
template <class KERNEL, class OUT, class... REST>
inline int launch_over_column(KERNEL kernel, uint64_t n_wg, dim3 block, unsigned lds_bytes, hipStream_t stream, const alpgpu_column* col, OUT out, REST... rest) {
	launch_in_grid_chunks(n_wg, [&](dim3 grid, uint64_t off) {
		hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, col->d_vectors, col->d_rowgroups, col->d_packed, col->d_exc, out, col->n_vectors, off, rest...);
	});
	return hipGetLastError() == hipSuccess ? ALPGPU_OK : ALPGPU_ERR_HIP;
}

// what alpgpu_encode_* memsets the rowgroup states to in front of a search that PUBLISHES them beside the encode: every byte 0xFF = "not there"
// (alp_device.hpp: rowgroup_state_is_whole — no word of a real state is all-ones, so a torn read of a state being published is recognised)
constexpr int kStateUnpublished = 0xFF;

// decode_kernels.hip
// progress (nullable): a word of device memory the kernel's workgroups report their position to, tagged (read_ahead_kernels.hip)
// gate (unhinted decode, api_decode.hip): != 0 -> the launch runs only if the context's shape word (progress[kCtxWordShape], decode_policy.hpp) holds this value
int launch_decode_column(hipStream_t stream, const alpgpu_column* col, double* d_out, const DecodeShape& shape, int n_cus, uint64_t* progress = nullptr, uint64_t progress_tag = 0,
                         uint32_t gate = 0);
// read_ahead_kernels.hip: the column's descriptors, packed words and exception records read into the Infinity Cache a bounded distance ahead of the decode
// kernel that reports to d_progress with this tag (lead_min / lead_max in vectors; value_bytes 8 or 4; grid workgroups of four wavefronts)
// ps_per_vector: picoseconds the decode needs per vector AT LEAST (the read-ahead's workgroups sleep by it between looks at the progress word);
// ps_per_tick: of wall_clock64() on this device (hipDeviceAttributeWallClockRate)
// d_ctx_words: the context's 2 KiB of device words (decode_policy.hpp); from_plan: lead, pace and max_bits are read from its plan words (an unhinted decode)
int launch_read_ahead(hipStream_t stream, const alpgpu_column* col, int value_bytes, uint64_t* d_ctx_words, uint64_t tag, uint32_t lead_min, uint32_t lead_max,
                      uint32_t ps_per_vector, uint32_t ps_per_tick, uint32_t max_bits, int grid, bool from_plan = false); // max_bits: records of wider vectors are left alone (their descriptors are read)
int launch_decode_sum(hipStream_t stream, const alpgpu_column* col, double* d_sums, int vectors_per_wg);
int launch_decode_count_range(hipStream_t stream, const alpgpu_column* col, double lo, double hi, uint32_t* d_counts);
// the same sinks, one wavefront per vector, packed words straight from HBM (no stage, no barrier); count = false: per-vector sums (double), true: counts (u32)
int launch_sink_direct(hipStream_t stream, const alpgpu_column* col, double lo, double hi, void* d_out, bool count);
int launch_decode_sum_f32(hipStream_t stream, const alpgpu_column* col, double* d_sums);
int launch_decode_count_range_f32(hipStream_t stream, const alpgpu_column* col, float lo, float hi, uint32_t* d_counts);
int launch_sink_direct_f32(hipStream_t stream, const alpgpu_column* col, float lo, float hi, void* d_out, bool count);

// consume_kernels.hip: decode fused into SUM / COUNT consumers (persistent, software-pipelined), and the column total's tree
int launch_consume_sum(hipStream_t stream, const alpgpu_column* col, double* d_sums, int n_cus);
int launch_consume_count_range(hipStream_t stream, const alpgpu_column* col, double lo, double hi, uint32_t* d_counts, int n_cus);
int launch_tree_sum(hipStream_t stream, const double* d_in, uint64_t n, double* d_scratch, double* d_total);

// gather_kernels.hip: d_out[k] = value d_idx[k] of the column (d_idx != nullptr; out of range: the canonical quiet NaN) or value first + k (d_idx ==
// nullptr; the caller checked the range), k < n; value_bytes 8 or 4
int launch_gather(hipStream_t stream, const alpgpu_column* col, const int64_t* d_idx, uint64_t first, uint64_t n, void* d_out, int value_bytes);

// select_kernels.hip: the value indices r of [first, first + n) (n > 0, range checked by the caller) whose value x has lo <= x <= hi, ascending, into
// d_idx (and the values into d_vals, nullable) up to capacity; *d_count = how many qualify; d_scratch: select_scratch_bytes(col->n_vectors) bytes
uint64_t select_scratch_bytes(uint64_t n_vectors);
int launch_select_range(hipStream_t stream, const alpgpu_column* col, uint64_t first, uint64_t n, double lo, double hi, int64_t* d_idx, void* d_vals, uint64_t capacity,
                        uint64_t* d_count, void* d_scratch, int value_bytes, const void* d_zones = nullptr);
// ... its scan alone: d_offsets[i] = d_counts[0] + ... + d_counts[i - 1], *d_total = the sum of all n (n > 0); d_levels: select_scratch_bytes(n) bytes suffice
int launch_select_scan(hipStream_t stream, const uint32_t* d_counts, uint64_t n, uint64_t* d_offsets, uint64_t* d_total, uint64_t* d_levels);

// mask_kernels.hip: selection bitmaps (16 u64 words per vector, bit r & 63 of word r >> 6 = value index r).  launch_select_mask: bit(r) = / &= / |= q(r),
// q(r) = first <= r < first + n and lo <= x_r <= hi (n > 0, range and op checked by the caller); launch_mask_to_indices: the set bits as ascending
// indices up to capacity, *d_count = how many (n_vectors > 0; d_scratch: select_scratch_bytes(n_vectors) bytes); launch_sum_masked: d_sums[v] = the sum of
// the vector's values whose bit is set, d_counts[v] (nullable) = its set bits (col->n_vectors > 0); launch_decode_masked: the values at the set bits,
// ascending, into d_vals (and their indices into d_idx, nullable) up to capacity, *d_count = how many (col->n_vectors > 0, d_vals non-null when capacity > 0).
// launch_fill_u64: d_words[i] = value, i < n_words (> 0), by a kernel and not hipMemsetAsync (mask_kernels.hip, k_fill_u64, says why)
int launch_fill_u64(hipStream_t stream, uint64_t* d_words, uint32_t n_words, uint64_t value);
int launch_select_mask(hipStream_t stream, const alpgpu_column* col, uint64_t first, uint64_t n, double lo, double hi, int op, uint64_t* d_mask, int value_bytes);
int launch_mask_to_indices(hipStream_t stream, const uint64_t* d_mask, uint64_t n_vectors, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch);
int launch_sum_masked(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts, int value_bytes);
int launch_decode_masked(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, void* d_vals, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch,
                         int value_bytes);

// pair_kernels.hip: two columns of equal length (a->n_vectors == b->n_vectors > 0; a == b allowed), decoded side by side by one wavefront per
// vector pair.  launch_compare_mask: bit(r) = / &= / |= q(r), q(r) = first <= r < first + n and a_r CMP b_r (n > 0; range, cmp = ALPGPU_CMP_* and op
// checked by the caller); launch_dot_masked: d_sums[v] = the sum of a_r * b_r over the vector's set bits, d_counts[v] (nullable) = its set bits
int launch_compare_mask(hipStream_t stream, const alpgpu_column* a, const alpgpu_column* b, uint64_t first, uint64_t n, int cmp, int op, uint64_t* d_mask, int value_bytes);
int launch_dot_masked(hipStream_t stream, const alpgpu_column* a, const alpgpu_column* b, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts, int value_bytes);

// group_kernels.hip: grouped aggregation (val->n_vectors == key->n_vectors > 0; val == key allowed; 1 <= n_groups <= ALPGPU_GROUP_MAX).
// launch_group_sum: d_sums[g * n_vectors + v] = the sum of val_r over the vector's set bits whose key_r lies in [lo[g], hi[g]] (host arrays, read
// before the call returns; a float column's bounds are floats widened), d_counts (nullable) their number; launch_group_totals: row g of d_sums
// [n_groups][n] by launch_tree_sum's tree into d_total_sums[g], row g of d_counts (nullable with d_total_counts) added exactly (n > 0; d_scratch:
// 32 * n_groups * ceil(n / 1024) bytes, 16-byte aligned, read only when n > 1024)
int launch_group_sum(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const double* lo, const double* hi, uint32_t n_groups,
                     double* d_sums, uint32_t* d_counts, int value_bytes);
int launch_group_totals(hipStream_t stream, const double* d_sums, const uint32_t* d_counts, uint64_t n, uint32_t n_groups, double* d_total_sums, uint64_t* d_total_counts,
                        void* d_scratch);

// minmax_kernels.hip: masked and grouped MIN / MAX; value_bytes 8 or 4, d_zones records {min, max} of that type.  launch_minmax_masked:
// d_zones[v] = the record of the vector's values whose bit is set, d_counts[v] (nullable) = its set bits (col->n_vectors > 0);
// launch_group_minmax: the arguments of launch_group_sum, d_zones[g * n_vectors + v] = the record of val_r over the vector's set bits whose key_r
// lies in [lo[g], hi[g]], d_counts (nullable) their number; launch_group_minmax_totals: d_minmax[2 g], d_minmax[2 g + 1] = the reduction of row g
// of d_zones [n_groups][n] (n >= 0; no scratch)
int launch_minmax_masked(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, void* d_zones, uint32_t* d_counts, int value_bytes);
int launch_group_minmax(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const double* lo, const double* hi, uint32_t n_groups,
                        void* d_zones, uint32_t* d_counts, int value_bytes);
int launch_group_minmax_totals(hipStream_t stream, const void* d_zones, uint64_t n, uint32_t n_groups, void* d_minmax, int value_bytes);

// top_k_kernels.hip: ORDER BY x [DESC] LIMIT k under a bitmap.  top_k_layout: where the pieces of the caller's scratch lie (byte offsets, each a
// multiple of 16) and their total; false when n_vectors or k is more than the call accepts.  launch_top_k: col->n_vectors in 1 .. 2^32 - 1,
// 1 <= k <= ALPGPU_TOP_K_MAX, d_records nullable (then launch_minmax_masked writes them into the scratch), d_idx nullable; value_bytes 8 or 4.
// Memset, records, a histogram and a pick per digit of the vector level, the candidates, the same per digit of the element level, the filter, the sort.
struct TopKLayout {
	uint64_t records, counts, cand, stage, bins, state, total;
	uint64_t cand_capacity; // candidates: min(k, n_vectors) * 1024
};
inline bool top_k_layout(uint64_t n_vectors, uint64_t k, TopKLayout& L) {
	if (k > ALPGPU_TOP_K_MAX || n_vectors > 0xFFFFFFFFull) { return false; }
	const auto up16   = [](uint64_t x) { return (x + 15ull) & ~15ull; };
	L.cand_capacity   = (k < n_vectors ? k : n_vectors) * 1024ull;
	L.records         = 0;
	L.counts          = L.records + 16ull * n_vectors;
	L.cand            = L.counts + up16(4ull * n_vectors);
	L.stage           = L.cand + 16ull * L.cand_capacity;
	L.bins            = L.stage + 16ull * ALPGPU_TOP_K_MAX;
	L.state           = L.bins + 2ull * 16ull * 256ull * sizeof(uint32_t); // two levels of at most 16 passes
	L.total           = L.state + 64ull;
	return true;
}
int launch_top_k(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, const void* d_records, uint32_t k, int largest, void* d_vals, int64_t* d_idx,
                 uint64_t* d_count, void* d_scratch, int value_bytes);

// quantile_kernels.hip: the r-th smallest selected values under a bitmap.  quantile_layout: where the pieces of the caller's scratch lie (byte
// offsets, each a multiple of 16), their total and the candidate capacity, a function of n_vectors alone; false when n_vectors is more than the call
// accepts.  launch_quantile: col->n_vectors in 1 .. 2^32 - 1; q != nullptr: n quantiles in [0, 1] (n <= ALPGPU_QUANTILE_MAX; d_vals takes 2 n values,
// d_ranks, nullable, n ranks), else n ranks (n <= ALPGPU_RANK_MAX; d_vals takes n values); both host arrays, copied into the kernel arguments; d_zones
// nullable; tuning nullable (the debug entry's record).  quantile_trace: what the last call on this scratch did; synchronises the stream.
constexpr uint64_t kQuantileStateBytes = 2048;
struct QuantileLayout {
	uint64_t state, bins, cand, total;
	uint64_t capacity; // candidate keys: max(65536, 16 * n_vectors)
};
inline bool quantile_layout(uint64_t n_vectors, QuantileLayout& L) {
	if (n_vectors > 0xFFFFFFFFull) { return false; }
	L.capacity = 16ull * n_vectors > 65536ull ? 16ull * n_vectors : 65536ull;
	L.state    = 0;
	L.bins     = L.state + kQuantileStateBytes;
	L.cand     = L.bins + 8ull * ALPGPU_RANK_MAX * 256ull * sizeof(uint64_t); // at most 8 passes of 32 slots of 256 bins
	L.total    = L.cand + 8ull * L.capacity;
	return true;
}
int launch_quantile(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, const void* d_zones, const double* q, const uint64_t* ranks, uint32_t n, int from_top,
                    void* d_vals, uint64_t* d_ranks, uint64_t* d_count, void* d_scratch, int value_bytes, int n_cus, const alpgpu_quantile_tuning* tuning);
int quantile_trace(hipStream_t stream, const void* d_scratch, alpgpu_quantile_trace* out);

// in_list_kernels.hip: set membership.  launch_select_in_mask: bit(r) = / &= / |= q(r), q(r) = first <= r < first + n and ((some j < n_list has
// d_list[j] == x_r) != negate) (n > 0; range, op, n_list <= 2^31 - 1 and the alignments checked by the caller; d_list sorted, device memory of the
// column's type, NULL with n_list == 0; d_zones nullable: the column's zone map); one launch of persistent workgroups, at most four per CU.
// (in_list_lds_max, the longest list the kernel holds whole in LDS, and what of a longer one is staged: persistent_launch.hpp)
int launch_select_in_mask(hipStream_t stream, const alpgpu_column* col, uint64_t first, uint64_t n, const void* d_list, uint64_t n_list, int negate, const void* d_zones, int op,
                          uint64_t* d_mask, int value_bytes, int n_cus);

// join_kernels.hip: join probe.  launch_join_probe: one row per set bit of d_mask (nullable: every index), ascending, up to capacity: d_pos = the
// position of the first key == x in d_keys (d_rows nullable: the payload there) or ALPGPU_JOIN_NO_MATCH, d_span (nullable) = the keys == x, d_idx
// (nullable) = the value index; *d_count = the set bits (col->n_vectors > 0; n_keys <= 2^31 - 1, d_pos non-null with capacity > 0, d_scratch non-null with
// a bitmap and the alignments checked by the caller; d_keys sorted device memory of the column's type; d_zones nullable).  With a bitmap the popcount
// pass and the scan of mask_kernels.hip, then one launch of persistent workgroups, at most four per CU.  A call that launches no probe (capacity == 0
// without a bitmap) writes its count by launch_fill_u64.
int launch_join_probe(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, const void* d_zones, const void* d_keys, uint64_t n_keys, const int64_t* d_rows,
                      int64_t* d_pos, uint32_t* d_span, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch, int value_bytes, int n_cus);

// histogram_kernels.hip: bucket counts by sorted edges.  launch_histogram: d_counts[b] += the values x_r, r in [first, first + n) with its bit set in
// d_mask (nullable: every r), that are no NaNs and have b = #{i : d_edges[i] <= x_r} (right: <), d_counts[n_edges + 1] += those that are NaNs
// (col->n_vectors > 0, n > 0, n_edges <= ALPGPU_HISTOGRAM_EDGES_MAX; range and alignments checked by the caller, who has zeroed the counts unless they
// accumulate; d_edges sorted device memory of the column's type; d_zones, tuning and d_trace nullable); one launch of persistent workgroups, at most
// three per CU.  (A call that overwrites zeroes the counts first, by launch_fill_u64.)
int launch_histogram(hipStream_t stream, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const void* d_zones, const void* d_edges, uint32_t n_edges,
                     int right, uint64_t* d_counts, int value_bytes, int n_cus, const alpgpu_histogram_tuning* tuning, uint64_t* d_trace);

// distinct_kernels.hip: sorted distinct values and their counts.  distinct_layout: where the pieces of the caller's scratch lie (byte offsets, each a
// multiple of 16), their total and the table's sizes, a function of capacity alone (T = the power of two >= 2 * capacity slots of the global table, P =
// the power of two >= capacity pairs of the sort); false when capacity is 0 or beyond ALPGPU_DISTINCT_MAX.  launch_distinct: col->n_vectors > 0, n > 0,
// capacity in 1 .. ALPGPU_DISTINCT_MAX; range and alignments checked by the caller; d_counts, d_zones, tuning and d_trace nullable.  The reset, one
// launch of persistent workgroups (at most three per CU for float, two for double), the compaction, the sort's launches (their number a function of capacity and the tuning's
// sort_tile) and the emit, which writes d_state.  (A call without work zeroes the four words by launch_fill_u64.)
struct DistinctLayout {
	uint64_t state, keys, counts, pairs, total;
	uint64_t table_slots, sort_slots; // T, P
};
inline uint64_t distinct_pow2_at_or_above(uint64_t x) {
	uint64_t p = 1;
	while (p < x) { p <<= 1; }
	return p;
}
inline bool distinct_layout(uint64_t capacity, DistinctLayout& L) {
	if (capacity == 0 || capacity > ALPGPU_DISTINCT_MAX) { return false; }
	L.sort_slots  = distinct_pow2_at_or_above(capacity);
	L.table_slots = 2ull * L.sort_slots; // (the power of two >= 2 * capacity)
	L.state       = 0;
	L.keys        = L.state + 64ull;
	L.counts      = L.keys + 8ull * L.table_slots;
	L.pairs       = L.counts + 8ull * L.table_slots;
	L.total       = L.pairs + 16ull * L.sort_slots;
	return true;
}
int launch_distinct(hipStream_t stream, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const void* d_zones, uint64_t capacity, void* d_vals,
                    uint64_t* d_counts, uint64_t* d_state, void* d_scratch, int value_bytes, int n_cus, const alpgpu_distinct_tuning* tuning, uint64_t* d_trace);

// keyed_kernels.hip: SUM and COUNT per key of a sorted key list.  keyed_stripe_vectors: L, the vectors of a stripe; keyed_stripes: S = ceil(n_vectors / L)
// <= ALPGPU_KEYED_STRIPES_MAX, the rows of partials.  launch_keyed_sum: val->n_vectors == key->n_vectors in 1 .. 2^32 - 1 (val == key allowed), n_keys in
// 1 .. ALPGPU_KEYED_KEYS_MAX; the alignments checked by the caller; d_keys sorted device memory of the columns' type; d_mask, d_zones (the KEY column's
// records), d_counts (n_keys + 1 words), tuning and d_trace nullable; d_scratch: 64 bytes of header and S rows of n_keys doubles.  The init kernel, one
// launch of persistent workgroups (two per CU up to 256 keys, one beyond) and the reduce, one workgroup per key.
inline uint64_t keyed_stripe_vectors(uint64_t n_vectors) {
	const uint64_t l = n_vectors / ALPGPU_KEYED_STRIPES_MAX + (n_vectors % ALPGPU_KEYED_STRIPES_MAX != 0 ? 1u : 0u);
	return l > 0 ? l : 1;
}
inline uint64_t keyed_stripes(uint64_t n_vectors) {
	const uint64_t l = keyed_stripe_vectors(n_vectors);
	return n_vectors / l + (n_vectors % l != 0 ? 1u : 0u);
}
int launch_keyed_sum(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_keys, uint32_t n_keys,
                     double* d_sums, uint64_t* d_counts, void* d_scratch, int value_bytes, int n_cus, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);

// keyed_minmax_kernels.hip: the record {min, max} and the COUNT per key of a sorted key list.  launch_keyed_minmax_init: {+inf, -inf} into the n_keys
// records of d_out and 0 into the n_keys + 1 words of d_counts (nullable), by a kernel.  launch_keyed_minmax: launch_keyed_sum's arguments without a
// scratch, d_out n_keys records of the columns' type (value_bytes 8 or 4); the init kernel and one launch of persistent workgroups, two per CU.
int launch_keyed_minmax_init(hipStream_t stream, void* d_out, uint64_t* d_counts, uint32_t n_keys, int value_bytes);
int launch_keyed_minmax(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_keys, uint32_t n_keys,
                        void* d_out, uint64_t* d_counts, int value_bytes, int n_cus, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);

// keyed_minmax_many_kernels.hip: the same records and counts for n_keys in 1 .. ALPGPU_KEYED_MANY_KEYS_MAX: launch_keyed_minmax's arguments; the keys
// staged by list_staging's rule (persistent_launch.hpp), d_out and d_counts themselves the table.  launch_keyed_minmax_init and one launch of
// persistent workgroups, two per CU.
int launch_keyed_minmax_many(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_keys,
                             uint32_t n_keys, void* d_out, uint64_t* d_counts, int value_bytes, int n_cus, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);

// keyed_sum_exact_kernels.hip: the correctly rounded SUM and the COUNT per key for n_keys in 1 .. ALPGPU_KEYED_MANY_KEYS_MAX: launch_keyed_minmax_many's
// arguments with d_sums (n_keys doubles for both precisions) in place of the records, d_table (keyed_sum_exact_table_bytes(n_keys) bytes, 16-byte
// aligned: 66 limbs of int64 and a word of flags per key) and accumulate (0: a kernel zeroes the table and the counts first).  n_vectors may be 0.
// The zero kernel, one launch of persistent workgroups, two per CU, and the finish kernel that rounds every entry into d_sums.
uint64_t keyed_sum_exact_table_bytes(uint32_t n_keys);
int launch_keyed_sum_exact(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_keys,
                           uint32_t n_keys, double* d_sums, uint64_t* d_counts, void* d_table, int accumulate, int value_bytes, int n_cus, const alpgpu_keyed_tuning* tuning,
                           uint64_t* d_trace);

// bucket_kernels.hip: SUM, the record {min, max} and the COUNT per bucket of the key column by n_edges (0 .. ALPGPU_BUCKET_EDGES_MAX) sorted edges:
// launch_keyed_sum's / launch_keyed_minmax's arguments with d_edges (nullable with n_edges == 0) and `right` in place of the keys, n_edges + 1 sums or
// records, d_counts n_edges + 2 words, d_scratch 64 bytes of header and S rows of n_edges + 1 doubles; value_bytes 8 or 4 for both.
int launch_bucket_sum(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_edges, uint32_t n_edges,
                      int right, double* d_sums, uint64_t* d_counts, void* d_scratch, int value_bytes, int n_cus, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);
int launch_bucket_minmax(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const void* d_zones, const void* d_edges, uint32_t n_edges,
                         int right, void* d_out, uint64_t* d_counts, int value_bytes, int n_cus, const alpgpu_keyed_tuning* tuning, uint64_t* d_trace);

// zone maps (include/alpgpu.h).  decode_kernels.hip / decode_f32_kernels.hip: d_zones[v] = {min, max} of vector v, decoded in registers by the
// one-wavefront sink kernels (col->n_vectors > 0)
int launch_zone_map(hipStream_t stream, const alpgpu_column* col, void* d_zones);
int launch_zone_map_f32(hipStream_t stream, const alpgpu_column* col, void* d_zones);
// zone_kernels.hip: the same records from the raw values (n_vectors > 0), and the reduction of n records (n >= 0) to d_minmax[2]; value_bytes 8 or 4
int launch_zone_map_of_values(hipStream_t stream, const void* d_in, uint64_t n_vectors, void* d_zones, int value_bytes);
int launch_zones_minmax(hipStream_t stream, const void* d_zones, uint64_t n, void* d_minmax, int value_bytes);

// guard_kernels.hip
int launch_validate_column(hipStream_t stream, const alpgpu_column* col, uint32_t value_bytes, unsigned long long* d_first_bad);
int launch_count_rd_rowgroups(hipStream_t stream, const alpgpu_column* col, uint64_t* d_count);
// d_out[3 s .. 3 s + 2] = {packed bytes, exceptions, ALP_RD vectors} of segment s (seg_vectors consecutive vectors each)
int launch_segment_sums(hipStream_t stream, const alpgpu_column* col, uint64_t seg_vectors, uint32_t n_seg, uint64_t* d_out);
// the unhinted decode's plan (decode_policy.hpp: policy_unhinted) from the segment sums just taken, into the context's plan words; one small workgroup
int launch_unhinted_plan(hipStream_t stream, uint64_t* d_ctx_words, uint32_t n_seg, uint64_t n_vectors, int value_bytes, int read_ahead_option, int lead_us_option, uint32_t max_bits);

// init_kernels.hip
int launch_rowgroup_init(hipStream_t stream, const double* d_in, uint64_t n_vectors, alpgpu_rowgroup_state* d_rgs, uint16_t* d_rd_order, uint64_t rg_first = 0,
                         uint64_t rg_count = 0);

int launch_state_from_samples(hipStream_t stream, const double* d_samples, uint32_t n_samples, alpgpu_rowgroup_state* d_state, int force_rd, double* d_cut_estimate = nullptr);
// the persistent, publishing form (runs beside the single-pass encode on a second stream) and the tag clean-up behind it
// tile_shaped: eight-wavefront workgroups that fit a lean encode tile's slot (init_kernels.hip), else four wavefronts beside two classic tiles
int launch_rowgroup_init_async(hipStream_t stream, const double* d_in, uint64_t n_vectors, alpgpu_rowgroup_state* d_rgs, uint16_t* d_rd_order, uint64_t rg_first,
                               uint64_t rg_count, int grid, bool tile_shaped = false, uint32_t adaptive_base = 0);
// adaptive_base != 0: `grid` workgroups are launched, those beyond adaptive_base leave at once unless the column's head is mostly ALP_RD (init_kernels.hip)
int launch_rowgroup_init_async_f32(hipStream_t stream, const float* d_in, uint64_t n_vectors, alpgpu_rowgroup_state* d_rgs, uint16_t* d_rd_order, uint64_t rg_first,
                                   uint64_t rg_count, int grid);

// encode_kernels.hip
uint64_t encode_workspace_bytes(uint64_t n_vectors);
// single pass, k_encode_lean (encode_lean_kernels.hip: 6 KiB of LDS and <= 72 VGPRs per wavefront, three tiles per CU; force_stall: debug, every look-back
// that has to wait gives up — exercises the recovery route).  unordered: tiles reserve their bytes with one atomic add instead of waiting for their
// predecessors' sizes (ALPGPU_OPT_ENCODE_UNORDERED)
int launch_encode_fused(hipStream_t stream, const double* d_in, uint64_t n_vectors, const alpgpu_column* col, uint64_t* d_workspace, bool force_stall = false,
                        bool async_states = false, hipEvent_t async_join = nullptr, hipEvent_t async_head = nullptr, bool unordered = false);
// pieces of the above for a caller that interleaves other work: zero d_totals, then vector ranges in ascending order
int launch_encode_reset_totals(hipStream_t stream, const alpgpu_column* col);
int launch_encode_fused_range(hipStream_t stream, const double* d_in, const alpgpu_column* col, uint64_t* d_workspace, uint64_t v_first, uint64_t n_range,
                              bool force_stall = false, bool async_states = false, hipEvent_t async_join = nullptr, hipEvent_t async_head = nullptr,
                              bool unordered = false);
// two pass; gate = nullptr: unconditionally, else a device word that must be non-zero for the kernels to do anything (d_totals + 6)
int launch_encode_vectors(hipStream_t stream, const double* d_in, uint64_t n_vectors, const alpgpu_column* col, uint64_t* d_workspace,
                          int n_cus, const uint64_t* gate = nullptr);
int launch_scan_offsets(hipStream_t stream, const alpgpu_column* col, uint64_t n_vectors, uint64_t* d_workspace, bool f32, const uint64_t* gate);

// pad_kernels.hip
int launch_pad_tail(hipStream_t stream, double* d_in, uint64_t n_values);

// primitive_kernels.hip
int launch_ffor_i64(hipStream_t stream, int n_cus, const int64_t* in, int64_t* packed, size_t stride, const uint8_t* bw,
                    const int64_t* base, uint64_t n);
int launch_unffor_i64(hipStream_t stream, int n_cus, const int64_t* packed, size_t stride, int64_t* out, const uint8_t* bw,
                      const int64_t* base, uint64_t n);
int launch_falp(hipStream_t stream, int n_cus, const int64_t* packed, size_t stride, double* out, const uint8_t* bw,
                const int64_t* base, const uint8_t* fac, const uint8_t* exp, uint64_t n);
int launch_ffor_u16(hipStream_t stream, int n_cus, const uint16_t* in, uint16_t* packed, size_t stride, const uint8_t* bw,
                    const uint16_t* base, uint64_t n);
int launch_unffor_u16(hipStream_t stream, int n_cus, const uint16_t* packed, size_t stride, uint16_t* out, const uint8_t* bw,
                      const uint16_t* base, uint64_t n);
int launch_ffor_u8(hipStream_t stream, int n_cus, const uint8_t* in, uint8_t* packed, size_t stride, const uint8_t* bw, const uint8_t* base, uint64_t n);
int launch_unffor_u8(hipStream_t stream, int n_cus, const uint8_t* packed, size_t stride, uint8_t* out, const uint8_t* bw, const uint8_t* base, uint64_t n);
int launch_decode_values(hipStream_t stream, int n_cus, const int64_t* enc, double* out, const uint8_t* fac, const uint8_t* exp,
                         uint64_t n);
int launch_patch(hipStream_t stream, int n_cus, double* out, const double* exc, const uint16_t* pos, size_t stride,
                 const uint16_t* cnt, uint64_t n);
int launch_analyze_ffor(hipStream_t stream, int n_cus, const int64_t* enc, uint8_t* bw, int64_t* base, uint64_t n);
int launch_encode_simdized(hipStream_t stream, int n_cus, const double* in, double* exc, uint16_t* pos, size_t stride, uint16_t* cnt,
                           int64_t* enc, const uint8_t* fac, const uint8_t* exp, uint64_t n);
int launch_encode_value(hipStream_t stream, const double* in, int64_t* enc, int fac, int exp, int safe, uint64_t n);
int launch_encode_value_f32(hipStream_t stream, const float* in, int32_t* enc, int fac, int exp, uint64_t n);
int launch_decode_probe(hipStream_t stream, const alpgpu_column* col, double* d_sums);
int launch_traffic_probe(hipStream_t stream, const void* d_in, void* d_out, uint64_t n_vectors, uint32_t write_bytes);
int launch_encode_values(hipStream_t stream, int n_cus, const double* in, const alpgpu_rowgroup_state* states, const uint32_t* idx,
                         double* exc, uint16_t* pos, size_t stride, uint16_t* cnt, int64_t* enc, uint8_t* fac, uint8_t* exp, uint64_t n);
int launch_rd_encode(hipStream_t stream, int n_cus, const double* in, const alpgpu_rowgroup_state* states, const uint32_t* idx,
                     uint16_t* exc, uint16_t* pos, size_t stride, uint16_t* cnt, uint64_t* right, uint16_t* left, uint64_t n);
int launch_rd_decode(hipStream_t stream, int n_cus, double* out, const uint64_t* right, const uint16_t* left,
                     const alpgpu_rowgroup_state* states, const uint32_t* idx, const uint16_t* exc, const uint16_t* pos, size_t stride,
                     const uint16_t* cnt, uint64_t n);


// ---- single precision (decode_f32_kernels.hip, encode_f32_kernels.hip, init_kernels.hip, primitive_f32_kernels.hip) ----
// shape: staged or one wavefront per vector (a streamed one goes to launch_decode_stream_f32); progress / tag / gate: as launch_decode_column
int launch_decode_column_f32(hipStream_t stream, const alpgpu_column* col, float* d_out, const DecodeShape& shape, uint64_t* progress = nullptr, uint64_t progress_tag = 0, uint32_t gate = 0);
// decode_stream_f32_kernels.hip: persistent workgroups, three chunks in flight each; shape 16: chunks of 8 vectors / 8 KiB of records, 17: 16 / 16 KiB, 18: 4 / 12 KiB
int launch_decode_stream_f32(hipStream_t stream, const alpgpu_column* col, float* d_out, int shape, int n_cus, uint64_t* progress = nullptr, uint64_t progress_tag = 0);
int launch_rowgroup_init_f32(hipStream_t stream, const float* d_in, uint64_t n_vectors, alpgpu_rowgroup_state* d_rgs, uint16_t* d_rd_order,
                             uint64_t rg_first = 0, uint64_t rg_count = 0);
int launch_state_from_samples_f32(hipStream_t stream, const float* d_samples, uint32_t n_samples, alpgpu_rowgroup_state* d_state, int force_rd, double* d_cut_estimate = nullptr);
int launch_encode_fused_f32(hipStream_t stream, const float* d_in, uint64_t n_vectors, const alpgpu_column* col, uint64_t* d_workspace, bool force_stall = false,
                            bool async_states = false, hipEvent_t async_join = nullptr, hipEvent_t async_head = nullptr, bool unordered = false);
int launch_encode_fused_range_f32(hipStream_t stream, const float* d_in, const alpgpu_column* col, uint64_t* d_workspace, uint64_t v_first, uint64_t n_range,
                                  bool force_stall = false, bool async_states = false, hipEvent_t async_join = nullptr, hipEvent_t async_head = nullptr,
                                  bool unordered = false);
int launch_encode_vectors_f32(hipStream_t stream, const float* d_in, uint64_t n_vectors, const alpgpu_column* col, uint64_t* d_workspace, const uint64_t* gate = nullptr);
int launch_pad_tail_f32(hipStream_t stream, float* d_in, uint64_t n_values);
int launch_ffor_i32(hipStream_t stream, int n_cus, const int32_t* in, int32_t* packed, size_t stride, const uint8_t* bw, const int32_t* base, uint64_t n);
int launch_unffor_i32(hipStream_t stream, int n_cus, const int32_t* packed, size_t stride, int32_t* out, const uint8_t* bw, const int32_t* base, uint64_t n);
int launch_falp_f32(hipStream_t stream, int n_cus, const int32_t* packed, size_t stride, float* out, const uint8_t* bw, const int32_t* base,
                    const uint8_t* fac, const uint8_t* exp, uint64_t n);
int launch_decode_values_f32(hipStream_t stream, int n_cus, const int32_t* enc, float* out, const uint8_t* fac, const uint8_t* exp, uint64_t n);
int launch_patch_f32(hipStream_t stream, int n_cus, float* out, const float* exc, const uint16_t* pos, size_t stride, const uint16_t* cnt, uint64_t n);
int launch_analyze_ffor_i32(hipStream_t stream, int n_cus, const int32_t* enc, uint8_t* bw, int32_t* base, uint64_t n);
int launch_encode_simdized_f32(hipStream_t stream, int n_cus, const float* in, float* exc, uint16_t* pos, size_t stride, uint16_t* cnt, int32_t* enc,
                               const uint8_t* fac, const uint8_t* exp, uint64_t n);
int launch_encode_values_f32(hipStream_t stream, int n_cus, const float* in, const alpgpu_rowgroup_state* states, const uint32_t* idx, float* exc,
                             uint16_t* pos, size_t stride, uint16_t* cnt, int32_t* enc, uint8_t* fac, uint8_t* exp, uint64_t n);
int launch_rd_encode_f32(hipStream_t stream, int n_cus, const float* in, const alpgpu_rowgroup_state* states, const uint32_t* idx, uint16_t* exc,
                         uint16_t* pos, size_t stride, uint16_t* cnt, uint32_t* right, uint16_t* left, uint64_t n);
int launch_rd_decode_f32(hipStream_t stream, int n_cus, float* out, const uint32_t* right, const uint16_t* left, const alpgpu_rowgroup_state* states,
                         const uint32_t* idx, const uint16_t* exc, const uint16_t* pos, size_t stride, const uint16_t* cnt, uint64_t n);

} // namespace alpgpu
