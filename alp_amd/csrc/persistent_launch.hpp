// persistent_launch.hpp — the host's two launch rules of the persistent scan kernels (k_in_list, k_join_probe, k_histogram, k_distinct_insert,
// k_quantile_wide, k_keyed_minmax_many, and k_keyed_sum and k_keyed_minmax, which take the grid rule only), stated once: how many workgroups a launch has, and what of a sorted list a workgroup stages into LDS.  Pure functions of
// numbers and plain C++ without a HIP type, as decode_policy.hpp is: tests/cpp/persistent_launch_test.cpp holds them without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace alpgpu {

constexpr uint32_t kTuningGridMax = 1u << 16; // of a tuning record's grid

// The grid of a launch whose workgroups of `waves` wavefronts walk `vectors` vectors, one per wavefront and trip: a workgroup per `waves` vectors,
// but no more than the device holds at once (n_cus * wg_per_cu; n_cus <= 0 counts as 1), since a workgroup sets its LDS up once and then stays.
// resident_cap (0: none) may only lower what the device holds.  grid_override (0: none) is a tuning record's grid: it replaces the rule's,
// clamped to override_max (a grid beyond the vectors: workgroups that find none).  (k_keyed_sum passes its STRIPES as `vectors`: a wavefront
// takes a stripe of consecutive vectors per trip, so the units of work the rule counts are stripes there.)
inline unsigned persistent_grid(uint64_t vectors, uint32_t waves, int n_cus, uint32_t wg_per_cu, uint64_t resident_cap = 0, uint32_t grid_override = 0,
                                uint32_t override_max = kTuningGridMax) {
	if (grid_override != 0u) { return grid_override < override_max ? grid_override : override_max; }
	const uint64_t n_wg     = (vectors + waves - 1) / waves;
	uint64_t       resident = static_cast<uint64_t>(n_cus > 0 ? n_cus : 1) * wg_per_cu;
	if (resident_cap != 0 && resident_cap < resident) { resident = resident_cap; }
	return static_cast<unsigned>(n_wg < resident ? n_wg : resident);
}

// The sorted list of k_in_list, k_join_probe and k_keyed_minmax_many (sorted_list.hpp) has 32 KiB of LDS per workgroup.  in_list_lds_max: the longest list that sits
// there whole (value_bytes 8 or 4; else 0).  A longer one is staged as its pivots, every stride-th element: LDS word i = list[i * stride].
constexpr uint32_t kInLdsBytes = 32768; // 4096 doubles or 8192 floats; with the exception masks 33 KiB, four workgroups per CU
inline size_t in_list_lds_max(int value_bytes) { return value_bytes == 8 || value_bytes == 4 ? kInLdsBytes / static_cast<uint32_t>(value_bytes) : 0u; }

struct ListStaging { // of list_staging(n_list <= 2^31 - 1, value_bytes 8 or 4)
	uint32_t stride; // 1: the list itself is staged
	uint32_t n_piv;  // LDS words staged: ceil(n_list / stride) <= in_list_lds_max
};
inline ListStaging list_staging(uint64_t n_list, int value_bytes) {
	const uint64_t lds_max = in_list_lds_max(value_bytes);
	ListStaging    s;
	s.stride = n_list > lds_max ? static_cast<uint32_t>((n_list + lds_max - 1) / lds_max) : 1u;
	s.n_piv  = static_cast<uint32_t>((n_list + s.stride - 1) / s.stride);
	return s;
}

} // namespace alpgpu
