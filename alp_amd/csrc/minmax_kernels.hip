// minmax_kernels.hip — masked and grouped MIN / MAX (include/alpgpu.h): zone records over the values a bitmap selects, per vector and per group
// of a key column, and every group's column MIN / MAX.
//
//   alpgpu_decode_minmax_masked_*  k_minmax_masked<VB> (minmax_device.hpp): one wavefront decodes vector v in registers and keeps the minimum and
//                                  maximum of the values whose bit is set.
//   alpgpu_decode_group_minmax_*   k_group_minmax<VB, GT>: k_group's skeleton with a {min, max} pair per group instead of a sum.  GT = 4, 8 or 16 is
//                                  the smallest tier that holds n_groups; the bounds travel as kernel arguments, the unused ones padded with lo > hi.
//   alpgpu_group_minmax_totals_*   k_group_zones_reset / k_group_zones_reduce: the reset and the reduction of alpgpu_zones_minmax_*
//                                  (zone_kernels.hip) with the group in the grid's second dimension.  No scratch.
//
// HBM traffic per vector: the bitmap's 128 bytes and, unless they settle the vector, the descriptors, packed words and exception records of the
// column (grouped: of both columns); 16 or 8 (+ 4) bytes written per group.  One launch, split only at the grid limit.
#include "launch.hpp"
#include "minmax_device.hpp"

namespace alpgpu {

// col->n_vectors > 0 (the caller checked)
int launch_minmax_masked(hipStream_t stream, const alpgpu_column* col, const uint64_t* d_mask, void* d_zones, uint32_t* d_counts, int value_bytes) {
	MinmaxArgs args {};
	args.n_vectors = col->n_vectors;
	args.mask      = d_mask;
	args.zones     = d_zones;
	args.counts    = d_counts;
	const ColumnStreams c = column_streams(col);
	return launch_vectors(args.n_vectors, kSelWaves, [&](dim3 grid, uint64_t off) {
		args.wg_off = off;
		if (value_bytes == 8) {
			hipLaunchKernelGGL((k_minmax_masked<8>), grid, dim3(kSelThreads), 0, stream, c, args);
		} else {
			hipLaunchKernelGGL((k_minmax_masked<4>), grid, dim3(kSelThreads), 0, stream, c, args);
		}
	});
}

template <int VB>
static int group_minmax(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, MinmaxArgs args, const double* lo, const double* hi) {
	const ColumnStreams cv = column_streams(val), ck = column_streams(key);
	return with_group_tier<VB>(lo, hi, args.n_groups, [&](auto r) {
		return launch_vectors(args.n_vectors, kSelWaves, [&](dim3 grid, uint64_t off) {
			args.wg_off = off;
			hipLaunchKernelGGL((k_group_minmax<VB, decltype(r)::kTier>), grid, dim3(kSelThreads), 0, stream, cv, ck, args, r);
		});
	});
}

// val->n_vectors == key->n_vectors > 0, 1 <= n_groups <= ALPGPU_GROUP_MAX (the caller checked)
int launch_group_minmax(hipStream_t stream, const alpgpu_column* val, const alpgpu_column* key, const uint64_t* d_mask, const double* lo, const double* hi, uint32_t n_groups,
                        void* d_zones, uint32_t* d_counts, int value_bytes) {
	MinmaxArgs args {};
	args.n_vectors = val->n_vectors;
	args.mask      = d_mask;
	args.zones     = d_zones;
	args.counts    = d_counts;
	args.n_groups  = n_groups;
	return value_bytes == 8 ? group_minmax<8>(stream, val, key, args, lo, hi) : group_minmax<4>(stream, val, key, args, lo, hi);
}

// ---- the groups' totals -------------------------------------------------------------------------------------------------------------------------
constexpr int      kTotalsThreads = 256;
constexpr unsigned kTotalsGrid    = 2048; // workgroups per group at most: two atomics each

template <class T>
__global__ void k_group_zones_reset(T* __restrict__ d_minmax, uint32_t n_groups) {
	if (threadIdx.x < n_groups) {
		d_minmax[2u * threadIdx.x]      = pos_inf<T>();
		d_minmax[2u * threadIdx.x + 1u] = -pos_inf<T>();
	}
}

// k_zones_reduce (zone_kernels.hip) for row blockIdx.y of zones[gridDim.y][n]: a grid-stride pass, one pair of candidates per workgroup, joined
// to d_minmax[2 g], d_minmax[2 g + 1] (reset in front of this launch) by two atomics chosen by the candidate's sign
template <class T>
__global__ __launch_bounds__(kTotalsThreads) void k_group_zones_reduce(const T* __restrict__ zones, uint64_t n, T* __restrict__ d_minmax) {
	__shared__ T s_mn[kTotalsThreads / 64], s_mx[kTotalsThreads / 64];
	const T*     row = zones + 2ull * blockIdx.y * n;
	T            mn = pos_inf<T>(), mx = -pos_inf<T>();
	for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kTotalsThreads + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * kTotalsThreads) {
		T z_min, z_max; // one 16-byte (8-byte) load per record
		if constexpr (sizeof(T) == 8) {
			const double2 z = reinterpret_cast<const double2*>(row)[i];
			z_min = z.x, z_max = z.y;
		} else {
			const float2 z = reinterpret_cast<const float2*>(row)[i];
			z_min = z.x, z_max = z.y;
		}
		T unused_mx = -pos_inf<T>(), unused_mn = pos_inf<T>();
		minmax_take(mn, unused_mx, z_min); // (a record never holds a NaN; one that does is ignored like a NaN value)
		minmax_take(unused_mn, mx, z_max);
	}
	wave_minmax<T>(mn, mx);
	const uint32_t wave = threadIdx.x >> 6;
	if ((threadIdx.x & 63u) == 0u) {
		s_mn[wave] = mn;
		s_mx[wave] = mx;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		for (int w = 1; w < kTotalsThreads / 64; ++w) {
			T unused_mx = -pos_inf<T>(), unused_mn = pos_inf<T>();
			minmax_take(mn, unused_mx, s_mn[w]);
			minmax_take(unused_mn, mx, s_mx[w]);
		}
		atomic_min_value<T>(d_minmax + 2u * blockIdx.y, mn);
		atomic_max_value<T>(d_minmax + 2u * blockIdx.y + 1u, mx);
	}
}

template <class T>
static int group_minmax_totals(hipStream_t stream, const T* d_zones, uint64_t n, uint32_t n_groups, T* d_minmax) {
	hipLaunchKernelGGL((k_group_zones_reset<T>), dim3(1), dim3(64), 0, stream, d_minmax, n_groups);
	if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	if (n == 0) { return ALPGPU_OK; }
	const uint64_t blocks = (n + kTotalsThreads - 1) / kTotalsThreads;
	hipLaunchKernelGGL((k_group_zones_reduce<T>), dim3(blocks < kTotalsGrid ? static_cast<unsigned>(blocks) : kTotalsGrid, n_groups), dim3(kTotalsThreads), 0, stream, d_zones, n, d_minmax);
	return hipGetLastError() == hipSuccess ? ALPGPU_OK : ALPGPU_ERR_HIP;
}

// 1 <= n_groups <= ALPGPU_GROUP_MAX (the caller checked); n >= 0
int launch_group_minmax_totals(hipStream_t stream, const void* d_zones, uint64_t n, uint32_t n_groups, void* d_minmax, int value_bytes) {
	return value_bytes == 8 ? group_minmax_totals<double>(stream, static_cast<const double*>(d_zones), n, n_groups, static_cast<double*>(d_minmax))
	                        : group_minmax_totals<float>(stream, static_cast<const float*>(d_zones), n, n_groups, static_cast<float*>(d_minmax));
}

} // namespace alpgpu
