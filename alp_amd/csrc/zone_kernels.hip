// zone_kernels.hip — zone maps without a decode (include/alpgpu.h, section "zone maps"): the records of a raw column (alpgpu_zone_map_of_values_*)
// and the reduction of a zone map to the column's minimum and maximum (alpgpu_zones_minmax_*).  The records of an ENCODED column come from the
// one-wavefront sink kernels (decode_kernels.hip: k_sink_direct<kSinkMinMax>, decode_f32_kernels.hip: k_sink_direct_f32<kSinkMinMaxF>); the codec
// is lossless, so both routes give the same bytes.
//
// A record is {min, max} over the vector's values that are not NaN, with -0.0 below +0.0, {+inf, -inf} when there is none (wave_minmax.hpp).
//
// k_zone_of_values: one wavefront per vector, four per workgroup.  A lane reads 16 bytes per load, 64 lanes 1 KiB, eight (float: four) loads
// per vector, all requested before the first is used; min and max in registers, then wave_minmax_*; 16 (8) bytes written.  HBM traffic: the
// column once.
// k_zones_reduce: a grid-stride pass over the records, one pair of candidates per workgroup, which joins the result by two atomics.  The
// result holds VALUE bits at all times (it starts as {+inf, -inf}), so the atomic is chosen by the candidate's sign: among values without the
// sign bit the signed-integer order of the bits is the values' order, among values with it the unsigned order reversed, and any value with the
// sign bit (-0.0 included) lies below any without.  Minimum and maximum are associative and commutative, so the order in which workgroups
// arrive does not show in the result.
#include <type_traits>

#include "launch.hpp"
#include "wave_minmax.hpp"

namespace alpgpu {

constexpr int      kZoneWaves   = 4; // wavefronts per workgroup
constexpr int      kZoneThreads = 64 * kZoneWaves;
constexpr uint64_t kZoneMaxGrid = 1ull << 30;
constexpr unsigned kReduceGrid  = 2048; // workgroups of the reduction at most: two atomics each

template <class T>
__global__ __launch_bounds__(kZoneThreads) void k_zone_of_values(const T* __restrict__ in, uint64_t n_vectors, uint64_t wg_off, T* __restrict__ zones) {
	typedef T V16 __attribute__((ext_vector_type(16 / sizeof(T))));
	constexpr int kLoads = 1024 * sizeof(T) / (64 * 16);
	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t v    = (wg_off + blockIdx.x) * kZoneWaves + wave;
	if (v >= n_vectors) { return; } // wave-uniform
	const V16* p = reinterpret_cast<const V16*>(in + v * 1024ull);
	V16        x[kLoads];
#pragma unroll
	for (int m = 0; m < kLoads; ++m) { x[m] = __builtin_nontemporal_load(p + 64 * m + lane); } // read exactly once
	T mn = pos_inf<T>(), mx = -pos_inf<T>();
#pragma unroll
	for (int m = 0; m < kLoads; ++m) {
#pragma unroll
		for (int c = 0; c < static_cast<int>(16 / sizeof(T)); ++c) { minmax_take(mn, mx, x[m][c]); }
	}
	wave_minmax<T>(mn, mx);
	if (lane == 0u) {
		zones[2 * v]     = mn;
		zones[2 * v + 1] = mx;
	}
}

template <class T>
__global__ void k_zones_reset(T* __restrict__ d_minmax) {
	d_minmax[0] = pos_inf<T>();
	d_minmax[1] = -pos_inf<T>();
}

// d_minmax was reset by k_zones_reset in front of this launch
template <class T>
__global__ __launch_bounds__(kZoneThreads) void k_zones_reduce(const T* __restrict__ zones, uint64_t n, T* __restrict__ d_minmax) {
	__shared__ T s_mn[kZoneWaves], s_mx[kZoneWaves];
	T            mn = pos_inf<T>(), mx = -pos_inf<T>();
	for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kZoneThreads + threadIdx.x; i < n; i += static_cast<uint64_t>(gridDim.x) * kZoneThreads) {
		T z_min, z_max; // one 16-byte (8-byte) load per record
		if constexpr (sizeof(T) == 8) {
			const double2 z = reinterpret_cast<const double2*>(zones)[i];
			z_min = z.x, z_max = z.y;
		} else {
			const float2 z = reinterpret_cast<const float2*>(zones)[i];
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
		for (int w = 1; w < kZoneWaves; ++w) {
			T unused_mx = -pos_inf<T>(), unused_mn = pos_inf<T>();
			minmax_take(mn, unused_mx, s_mn[w]);
			minmax_take(unused_mn, mx, s_mx[w]);
		}
		atomic_min_value<T>(d_minmax, mn);
		atomic_max_value<T>(d_minmax + 1, mx);
	}
}

template <class T>
static int zone_map_of_values(hipStream_t stream, const T* d_in, uint64_t n_vectors, T* d_zones) {
	const uint64_t n_wg = (n_vectors + kZoneWaves - 1) / kZoneWaves;
	for (uint64_t off = 0; off < n_wg; off += kZoneMaxGrid) {
		const uint64_t g = n_wg - off < kZoneMaxGrid ? n_wg - off : kZoneMaxGrid;
		hipLaunchKernelGGL((k_zone_of_values<T>), dim3(static_cast<unsigned>(g)), dim3(kZoneThreads), 0, stream, d_in, n_vectors, off, d_zones);
		if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	}
	return ALPGPU_OK;
}

int launch_zone_map_of_values(hipStream_t stream, const void* d_in, uint64_t n_vectors, void* d_zones, int value_bytes) {
	return value_bytes == 8 ? zone_map_of_values<double>(stream, static_cast<const double*>(d_in), n_vectors, static_cast<double*>(d_zones))
	                        : zone_map_of_values<float>(stream, static_cast<const float*>(d_in), n_vectors, static_cast<float*>(d_zones));
}

template <class T>
static int zones_minmax(hipStream_t stream, const T* d_zones, uint64_t n, T* d_minmax) {
	hipLaunchKernelGGL((k_zones_reset<T>), dim3(1), dim3(1), 0, stream, d_minmax);
	if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	if (n == 0) { return ALPGPU_OK; }
	const uint64_t blocks = (n + kZoneThreads - 1) / kZoneThreads;
	hipLaunchKernelGGL((k_zones_reduce<T>), dim3(blocks < kReduceGrid ? static_cast<unsigned>(blocks) : kReduceGrid), dim3(kZoneThreads), 0, stream, d_zones, n, d_minmax);
	return hipGetLastError() == hipSuccess ? ALPGPU_OK : ALPGPU_ERR_HIP;
}

int launch_zones_minmax(hipStream_t stream, const void* d_zones, uint64_t n, void* d_minmax, int value_bytes) {
	return value_bytes == 8 ? zones_minmax<double>(stream, static_cast<const double*>(d_zones), n, static_cast<double*>(d_minmax))
	                        : zones_minmax<float>(stream, static_cast<const float*>(d_zones), n, static_cast<float*>(d_minmax));
}

} // namespace alpgpu
