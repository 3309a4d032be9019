// group_kernels.hip — grouped aggregation (include/alpgpu.h): per-group SUM and COUNT by ranges of a key column, under a selection bitmap.
//
//   alpgpu_decode_group_sum_*   k_group<VB, GT> (group_device.hpp): one wavefront decodes vector v of the value column and vector v of the key
//                               column in registers, as k_pair does, and settles every group in that pass.  GT = 4, 8 or 16 is the smallest tier
//                               that holds n_groups; the bounds travel as kernel arguments, the unused ones padded with lo > hi.
//   alpgpu_group_totals         k_group_tree: k_tree_sum's level (consume_kernels.hip; blocks of 1024, (e0 + e1) + (e2 + e3), the wave tree,
//                               (s0 + s1) + (s2 + s3)) with the group in the grid's second dimension, and the rows of counts added up exactly as
//                               integers beside it.  Levels of ceil(n / 1024) per group in the caller's scratch.
//
// HBM traffic per vector: the bitmap's 128 bytes and, unless they settle the vector, both vectors' descriptors, packed words and exception
// records; 8 (+ 4) bytes written per group.  One launch, split only at the grid limit.
#include "group_device.hpp"
#include "launch.hpp"

namespace alpgpu {

template <int VB>
static int group_sum(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, GroupArgs args, const double* lo, const double* hi) {
	const ColumnStreams cv = column_streams(val), ck = column_streams(key);
	return with_group_tier<VB>(lo, hi, args.n_groups, [&](auto r) {
		return launch_vectors(args.n_vectors, kSelWaves, [&](dim3 grid, uint64_t off) {
			args.wg_off = off;
			hipLaunchKernelGGL((k_group<VB, decltype(r)::kTier>), grid, dim3(kSelThreads), 0, stream, cv, ck, args, r);
		});
	});
}

// val->n_vectors == key->n_vectors > 0, 1 <= n_groups <= ALPGPU_GROUP_MAX (the caller checked)
int launch_group_sum(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const double* lo, const double* hi, uint32_t n_groups,
                     double* d_sums, uint32_t* d_counts, int value_bytes) {
	GroupArgs args {};
	args.n_vectors = val->n_vectors;
	args.mask      = d_mask;
	args.sums      = d_sums;
	args.counts    = d_counts;
	args.n_groups  = n_groups;
	return value_bytes == 8 ? group_sum<8>(stream, val, key, args, lo, hi) : group_sum<4>(stream, val, key, args, lo, hi);
}

// ---- the groups' totals -------------------------------------------------------------------------------------------------------------------------
// One level of the reduction for every group: block (b, g) adds elements [1024 b, 1024 b + 1024) of row g of `in` (absent elements count as +0.0)
// in k_tree_sum's order, out[g * out_stride + b] = that sum; and, with counts, the same elements of row g of `cin` as integers.  C: uint32_t on the
// first level (the caller's counts), uint64_t on the later ones.
template <class C>
__global__ __launch_bounds__(256) void k_group_tree(const double* __restrict__ in, const C* __restrict__ cin, uint64_t n, uint64_t in_stride, double* __restrict__ out,
                                                    uint64_t* __restrict__ cout, uint64_t out_stride) {
	__shared__ double   s_w[4];
	__shared__ uint64_t s_c[4];
	const uint64_t i0  = static_cast<uint64_t>(blockIdx.x) * 1024 + 4ull * threadIdx.x;
	const double*  row = in + blockIdx.y * in_stride;
	double         e[4];
#pragma unroll
	for (int j = 0; j < 4; ++j) { e[j] = i0 + j < n ? row[i0 + j] : 0.0; }
	const double w = wave_tree_sum_f64((e[0] + e[1]) + (e[2] + e[3]));
	if ((threadIdx.x & 63) == 0) { s_w[threadIdx.x >> 6] = w; }
	if (cin != nullptr) {
		const C* crow = cin + blockIdx.y * in_stride;
		uint64_t c    = 0;
#pragma unroll
		for (int j = 0; j < 4; ++j) { c += i0 + j < n ? static_cast<uint64_t>(crow[i0 + j]) : 0ull; }
#pragma unroll
		for (int s = 32; s > 0; s >>= 1) { c += __shfl_xor(c, s, 64); } // (integers: any order gives the same sum)
		if ((threadIdx.x & 63) == 0) { s_c[threadIdx.x >> 6] = c; }
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		out[blockIdx.y * out_stride + blockIdx.x] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
		if (cin != nullptr) { cout[blockIdx.y * out_stride + blockIdx.x] = s_c[0] + s_c[1] + s_c[2] + s_c[3]; }
	}
}

// d_scratch (n > 1024 only): four buffers of n_groups * ceil(n / 1024) elements of 8 bytes back to back, two of sums and two of counts.
// n > 0, 1 <= n_groups <= ALPGPU_GROUP_MAX; d_counts and d_total_counts NULL together
int launch_group_totals(hipStream_t stream, const double* d_sums, const uint32_t* d_counts, uint64_t n, uint32_t n_groups, double* d_total_sums, uint64_t* d_total_counts,
                        void* d_scratch) {
	const uint64_t l1      = (n + 1023) / 1024;
	double*        sbuf[2] = {static_cast<double*>(d_scratch), static_cast<double*>(d_scratch) + n_groups * l1};
	uint64_t*      cbuf[2] = {static_cast<uint64_t*>(d_scratch) + 2 * n_groups * l1, static_cast<uint64_t*>(d_scratch) + 3 * n_groups * l1};
	const bool     with_counts = d_counts != nullptr;
	const double*  src = d_sums;
	const void*    csrc = d_counts;
	uint64_t       stride = n;
	int            t = 0;
	bool           first = true;
	while (true) {
		const uint64_t blocks = (n + 1023) / 1024;
		const bool     last   = blocks == 1;
		double*        dst    = last ? d_total_sums : sbuf[t];
		uint64_t*      cdst   = !with_counts ? nullptr : last ? d_total_counts : cbuf[t];
		const uint64_t ostride = last ? 1 : l1;
		const dim3     grid(static_cast<unsigned>(blocks), n_groups);
		if (first) {
			hipLaunchKernelGGL(k_group_tree<uint32_t>, grid, dim3(256), 0, stream, src, static_cast<const uint32_t*>(csrc), n, stride, dst, cdst, ostride);
		} else {
			hipLaunchKernelGGL(k_group_tree<uint64_t>, grid, dim3(256), 0, stream, src, static_cast<const uint64_t*>(csrc), n, stride, dst, cdst, ostride);
		}
		if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
		if (last) { break; }
		src    = dst;
		csrc   = cdst;
		stride = l1;
		n      = blocks;
		first  = false;
		t ^= 1;
	}
	return ALPGPU_OK;
}

} // namespace alpgpu
