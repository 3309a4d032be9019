// mask_kernels.hip — selection bitmaps (include/alpgpu.h): a predicate's qualify mask kept as 16 words per vector instead of being counted away,
// so that a second column's predicate combines with it where the ballot is made, and what is left is listed or summed at the very end.
//
//   alpgpu_select_mask_*         k_select<VB, kSelMask> (select_device.hpp): one wavefront per vector, the decode of the selection with its 16
//                                ballots stored, SET / AND / OR with what the bitmap held.  A vector outside the range, an all-zero vector under AND
//                                and an all-ones vector under OR cost their 128 bytes of bitmap and nothing of the column.
//   alpgpu_mask_to_indices       k_mask_count (per-vector popcount) -> launch_select_scan (select_kernels.hip) -> k_mask_emit: three launches
//                                ordered by kernel boundaries.  A set bit's position = its vector's offset from the prefix sum + the set bits of
//                                the words before + v_mbcnt of its own word: ascending, and no atomic anywhere.
//   alpgpu_decode_sum_masked_*   k_select<VB, kSelSum>: the same decode, each lane adding the values whose bit is set; the order is in
//                                include/alpgpu.h and belongs to this entry point (the persistent consumer of consume_kernels.hip has its own).
//   alpgpu_decode_masked_*       k_mask_count -> launch_select_scan -> k_select<VB, kSelTake>: the projection of a column under a bitmap.
//                                The emit pass is the selection's with the predicate replaced by a bit test: a vector's values at its set bits,
//                                compacted at offsets[v] + rank (and their indices beside them, as k_mask_emit writes them).
//
// HBM traffic per vector: select_mask SET writes 128 bytes beside the selection's count pass; AND / OR read 128 first and read the column only
// for vectors the bitmap leaves open; mask_to_indices reads 128 + 128 (the second only where a bit is set) and the scan's 12; the masked SUM
// reads 128 and, where a bit is set, the vector, and writes 8 (+ 4); the masked projection reads 128 and the scan's 12, then, where a bit is set and
// the capacity not yet reached, 128 again and the vector (its packed words and exception values only for the halves of the vector that hold a bit),
// and writes 8 or 4 (+ 8) bytes per selected value.
#include "select_device.hpp"

namespace alpgpu {

// counts[v] = set bits of words 16 v .. 16 v + 15: 16 lanes per vector, one word each (a wavefront reads 512 consecutive bytes)
__global__ __launch_bounds__(256) void k_mask_count(const uint64_t* __restrict__ mask, uint64_t n_vectors, uint64_t wg_off, uint32_t* __restrict__ counts) {
	const uint64_t t = (wg_off + blockIdx.x) * 256ull + threadIdx.x; // the word
	const uint64_t v = t >> 4;
	uint32_t       c = v < n_vectors ? static_cast<uint32_t>(__builtin_popcountll(mask[t])) : 0u;
	for (int s = 8; s > 0; s >>= 1) { c += __shfl_xor(c, s, 16); }
	if ((threadIdx.x & 15u) == 0u && v < n_vectors) { counts[v] = c; }
}

// one wavefront per vector: the indices of its set bits at offsets[v] + rank, below the capacity
__global__ __launch_bounds__(kSelThreads) void k_mask_emit(const uint64_t* __restrict__ mask, uint64_t n_vectors, uint64_t wg_off, const uint32_t* __restrict__ counts,
                                                           const uint64_t* __restrict__ offsets, int64_t* __restrict__ d_idx, uint64_t capacity) {
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t v    = (wg_off + blockIdx.x) * kSelWaves + wave;
	if (v >= n_vectors) { return; }
	const uint32_t total = counts[v];
	if (total == 0u) { return; } // a vector without a set bit costs these four bytes
	const uint64_t out0 = offsets[v];
	if (out0 >= capacity) { return; }
	const uint64_t mine   = lane < 16u ? mask[16ull * v + lane] : 0ull;
	uint32_t       before = 0; // set bits of the words done (wave-uniform)
	for (uint32_t m = 0; m < 16u; ++m) {
		const uint64_t w = readlane64(mine, m);
		const uint64_t j = out0 + before + mbcnt64(w, 0u);
		if (((w >> lane) & 1ull) && j < capacity) { d_idx[j] = static_cast<int64_t>((v << 10) + 64u * m + lane); }
		before += static_cast<uint32_t>(__builtin_popcountll(w));
		if (before >= total || out0 + before >= capacity) { return; }
	}
}

// The library's "memset" of a few 64-bit words: words[i] = value, i < n_words.  What a call enqueues that zeroes its counts before it adds to them
// (alpgpu_histogram_*), or that writes a small result with no other launch (the join probe's count, the distinct call's state without work).  A
// kernel, not hipMemsetAsync: captured into a graph with torch, the memset's node was observed to leave non-zero words at replays that came after
// other work on the device (tools/probe_graph_memset.py shows it with alpgpu_memset alone, 24 bytes to 514 KiB; the cause is not established:
// DESIGN.md, "Histograms"), and these calls have to stay capturable.
__global__ __launch_bounds__(256) void k_fill_u64(uint64_t* __restrict__ words, uint32_t n_words, uint64_t value) { // n_words > 0
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i < n_words) { words[i] = value; }
}
int launch_fill_u64(hipStream_t stream, uint64_t* d_words, uint32_t n_words, uint64_t value) {
	hipLaunchKernelGGL(k_fill_u64, dim3((n_words + 255u) / 256u), dim3(256), 0, stream, d_words, n_words, value);
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

// n > 0, first + n <= n_vectors * 1024 and op one of the three (the caller checked).  SET and AND touch every vector of the column (bits outside
// the range clear), OR only those of the range (bits outside it stay).
int launch_select_mask(hipStream_t stream, const alpgpu_column* col, uint64_t first, uint64_t n, double lo, double hi, int op, uint64_t* d_mask, int value_bytes) {
	SelArgs a {};
	a.first   = first;
	a.end     = first + n;
	a.v0      = op == kMaskOr ? first >> 10 : 0ull;
	a.n_range = op == kMaskOr ? ((a.end - 1) >> 10) - a.v0 + 1 : col->n_vectors;
	a.lo      = lo;
	a.hi      = hi;
	a.mask    = d_mask;
	a.op      = op;
	return value_bytes == 8 ? launch_select<8, kSelMask>(stream, col, a) : launch_select<4, kSelMask>(stream, col, a);
}

// col->n_vectors > 0
int launch_sum_masked(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts, int value_bytes) {
	SelArgs a {};
	a.n_range    = col->n_vectors;
	a.mask_in    = d_mask;
	a.sums       = d_sums;
	a.sum_counts = d_counts;
	return value_bytes == 8 ? launch_select<8, kSelSum>(stream, col, a) : launch_select<4, kSelSum>(stream, col, a);
}

// the first two phases of mask_to_indices and of the masked projection: counts[v] = the vector's set bits, offsets = their exclusive prefix sum,
// *d_count = the bitmap's set bits (n_vectors > 0; the scratch laid out as the selection's); declared in select_device.hpp: the join probe's too
int launch_mask_count_scan(hipStream_t stream, const uint64_t* d_mask, uint64_t n_vectors, uint64_t* d_count, const SelScratch& s) {
	const int rc = launch_vectors(n_vectors, 16, [&](dim3 grid, uint64_t off) { // 256 words = 16 vectors per workgroup
		hipLaunchKernelGGL(k_mask_count, grid, dim3(256), 0, stream, d_mask, n_vectors, off, s.counts);
	});
	return rc != ALPGPU_OK ? rc : launch_select_scan(stream, s.counts, n_vectors, s.offsets, d_count, s.levels);
}

// n_vectors > 0; d_scratch: select_scratch_bytes(n_vectors) bytes, 16-byte aligned, laid out as the selection's
int launch_mask_to_indices(hipStream_t stream, const uint64_t* d_mask, uint64_t n_vectors, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch) {
	const SelScratch s  = select_scratch(d_scratch, n_vectors);
	const int        rc = launch_mask_count_scan(stream, d_mask, n_vectors, d_count, s);
	if (rc != ALPGPU_OK || capacity == 0) { return rc; }
	return launch_vectors(n_vectors, kSelWaves, [&](dim3 grid, uint64_t off) {
		hipLaunchKernelGGL(k_mask_emit, grid, dim3(kSelThreads), 0, stream, d_mask, n_vectors, off, static_cast<const uint32_t*>(s.counts), static_cast<const uint64_t*>(s.offsets), d_idx,
		                   capacity);
	});
}

// col->n_vectors > 0; d_vals non-null when capacity > 0, d_idx nullable; d_scratch as for launch_mask_to_indices
int launch_decode_masked(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, void* d_vals, int64_t* d_idx, uint64_t capacity, uint64_t* d_count,
                         void* d_scratch, int value_bytes) {
	const SelScratch s  = select_scratch(d_scratch, col->n_vectors);
	const int        rc = launch_mask_count_scan(stream, d_mask, col->n_vectors, d_count, s);
	if (rc != ALPGPU_OK || capacity == 0) { return rc; }
	SelArgs a {};
	a.n_range   = col->n_vectors;
	a.mask_in   = d_mask;
	a.counts_in = s.counts;
	a.offsets   = s.offsets;
	a.d_idx     = d_idx;
	a.d_vals    = d_vals;
	a.capacity  = capacity;
	return value_bytes == 8 ? launch_select<8, kSelTake>(stream, col, a) : launch_select<4, kSelTake>(stream, col, a);
}

} // namespace alpgpu
