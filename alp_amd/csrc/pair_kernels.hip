// pair_kernels.hip — two-column consumers (include/alpgpu.h): one wavefront decodes vector v of column A and vector v of column B in registers
// and combines them lane by lane, so that neither column's values reach HBM.
//
//   alpgpu_compare_mask_*        k_pair<VB, kPairCompare> (pair_device.hpp): a_r CMP b_r balloted step by step, the 16 ballots SET into / ANDed /
//                                ORed with the selection bitmap.  The skip rules are alpgpu_select_mask_*'s: a vector outside the range, an
//                                all-zero vector under AND and an all-ones vector under OR cost their 128 bytes of bitmap and nothing of either column.
//   alpgpu_decode_dot_masked_*   k_pair<VB, kPairDot>: each lane adds the products a_r * b_r whose bit is set, product and sum rounded
//                                separately; the order is in include/alpgpu.h.  A vector without a set bit costs its 128 bytes of bitmap.
//
// HBM traffic per vector: the bitmap's 128 bytes (compare SET writes them without reading), and, unless they settle the vector, both vectors'
// descriptors, packed words and exception records; the dot writes 8 (+ 4) bytes.  One launch each, split only at the grid limit.
#include "launch.hpp"
#include "pair_device.hpp"

namespace alpgpu {

template <int VB, int ARM>
static int launch_pair(hipStream_t stream, const alpgpu_column* a, const alpgpu_column* b, PairArgs args) {
	const ColumnStreams ca = column_streams(a), cb = column_streams(b);
	return launch_vectors(args.n_range, kSelWaves, [&](dim3 grid, uint64_t off) {
		args.wg_off = off;
		hipLaunchKernelGGL((k_pair<VB, ARM>), grid, dim3(kSelThreads), 0, stream, ca, cb, args);
	});
}

// n > 0, first + n <= n_vectors * 1024, cmp and op valid, a->n_vectors == b->n_vectors > 0 (the caller checked).  SET and AND touch every vector
// (bits outside the range clear), OR only those of the range (bits outside it stay).
int launch_compare_mask(hipStream_t stream, const alpgpu_column* a, const alpgpu_column* b, uint64_t first, uint64_t n, int cmp, int op, uint64_t* d_mask, int value_bytes) {
	static const uint32_t kAccept[6] = {kPairLt, kPairLt | kPairEq, kPairGt, kPairGt | kPairEq, kPairEq, kPairLt | kPairGt | kPairUn}; // ALPGPU_CMP_LT .. _NE
	const uint64_t        end        = first + n;
	PairArgs              args {};
	args.v0      = op == kMaskOr ? first >> 10 : 0ull;
	args.n_range = op == kMaskOr ? ((end - 1) >> 10) - args.v0 + 1 : a->n_vectors;
	args.first   = first;
	args.end     = end;
	args.mask    = d_mask;
	args.op      = op;
	args.accept  = kAccept[cmp];
	return value_bytes == 8 ? launch_pair<8, kPairCompare>(stream, a, b, args) : launch_pair<4, kPairCompare>(stream, a, b, args);
}

// a->n_vectors == b->n_vectors > 0
int launch_dot_masked(hipStream_t stream, const alpgpu_column* a, const alpgpu_column* b, const uint64_t* d_mask, double* d_sums, uint32_t* d_counts, int value_bytes) {
	PairArgs args {};
	args.n_range = a->n_vectors;
	args.mask    = const_cast<uint64_t*>(d_mask); // (the dot arm only reads it)
	args.sums    = d_sums;
	args.counts  = d_counts;
	return value_bytes == 8 ? launch_pair<8, kPairDot>(stream, a, b, args) : launch_pair<4, kPairDot>(stream, a, b, args);
}

} // namespace alpgpu
