// wave_minmax.hpp — wavefront-wide minimum and maximum in registers (gfx950): the reduction the encoders use for a vector's value range and the
// zone-map kernels (decode_kernels.hip, decode_f32_kernels.hip, zone_kernels.hip) and the masked MIN / MAX (minmax_device.hpp) for a vector's
// record; and what the reductions of records share (zone_kernels.hip, minmax_kernels.hip): the atomics that join a result in the records' order.
#pragma once
#include "alp_device.hpp"

namespace alpgpu {

// cross-lane copy of a double by DPP (register to register); lanes without a valid source lane keep their own value
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v) {
	const uint64_t b  = static_cast<uint64_t>(__double_as_longlong(v));
	int            lo = static_cast<int>(static_cast<uint32_t>(b)), hi = static_cast<int>(static_cast<uint32_t>(b >> 32));
	lo                = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false);
	hi                = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false);
	return __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo)));
}
// the same where EVERY lane has a source lane (rotations inside a 16-lane row): no old value to keep, so no register copy in front
template <int CTRL>
__device__ __forceinline__ double dpp_all_f64(double v) {
	const uint64_t b  = static_cast<uint64_t>(__double_as_longlong(v));
	int            lo = static_cast<int>(static_cast<uint32_t>(b)), hi = static_cast<int>(static_cast<uint32_t>(b >> 32));
	lo                = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
	hi                = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
	return __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(static_cast<uint32_t>(hi)) << 32) | static_cast<uint32_t>(lo)));
}
// NaN-ignoring minimum over each 16-lane row, left in every lane of the row (row_ror 1, 2, 4, 8: 3 instructions per step)
__device__ __forceinline__ double row_min_f64(double t) {
	t = fmin_num(t, dpp_all_f64<0x121>(t));
	t = fmin_num(t, dpp_all_f64<0x122>(t));
	t = fmin_num(t, dpp_all_f64<0x124>(t));
	t = fmin_num(t, dpp_all_f64<0x128>(t));
	return t;
}
__device__ __forceinline__ double f64_from_words(uint32_t lo, uint32_t hi) { return __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(hi) << 32) | lo)); }

// Wavefront-wide NaN-ignoring min and max, returned wave-uniform.  ONE reduction chain for both: max = -min(-x); v_permlane32_swap (CDNA4)
// puts the minimum candidates of lane pairs (i, i + 32) side by side in lanes 0..31 and the negated maximum candidates in lanes 32..63, so a
// single v_min_f64 folds 64 -> 32 for both, four row rotations reduce every 16-lane row, and one row_bcast:15 joins rows (0,1) and (2,3):
// lane 31 holds the minimum, lane 63 minus the maximum.  25 vector instructions; two separate row_shr / row_bcast scans were 64, a third of
// them register copies (a DPP move that leaves some lanes unwritten is tied to its old value).
__device__ __forceinline__ void wave_minmax_f64(double& mn, double& mx) {
	const uint64_t a = static_cast<uint64_t>(__double_as_longlong(mn)), b = static_cast<uint64_t>(__double_as_longlong(mx)) ^ 0x8000000000000000ull;
	const auto     lo = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(a), static_cast<uint32_t>(b), false, false);
	const auto     hi = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(a >> 32), static_cast<uint32_t>(b >> 32), false, false);
	double         t  = fmin_num(f64_from_words(lo[0], hi[0]), f64_from_words(lo[1], hi[1]));
	t                 = row_min_f64(t);
	t                 = fmin_num(t, dpp_f64<0x142, 0xa>(t)); // row_bcast:15 into rows 1 and 3
	const uint64_t r  = static_cast<uint64_t>(__double_as_longlong(t));
	const uint32_t a0 = __builtin_amdgcn_readlane(static_cast<uint32_t>(r), 31), a1 = __builtin_amdgcn_readlane(static_cast<uint32_t>(r >> 32), 31);
	const uint32_t b0 = __builtin_amdgcn_readlane(static_cast<uint32_t>(r), 63), b1 = __builtin_amdgcn_readlane(static_cast<uint32_t>(r >> 32), 63);
	mn = f64_from_words(a0, a1);
	mx = f64_from_words(b0, b1 ^ 0x80000000u);
}

// ---- single precision ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float fmin_num_f32(float a, float b) {
	float d;
	asm("v_min_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
	return d;
}
__device__ __forceinline__ float fmax_num_f32(float a, float b) {
	float d;
	asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
	return d;
}
template <int CTRL>
__device__ __forceinline__ float dpp_all_f32(float v) {
	return __uint_as_float(static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(__float_as_uint(v)), CTRL, 0xf, 0xf, true)));
}
// wave_minmax_f64 for floats: the same single chain (v_permlane32_swap, max = -min(-x), four row rotations, one row_bcast:15), one register
// per value.  Like the double form it relies on v_min_f32 ordering -0.0 below +0.0, which the sign flip turns into the maximum's order.
__device__ __forceinline__ void wave_minmax_f32(float& mn, float& mx) {
	const uint32_t a = __float_as_uint(mn), b = __float_as_uint(mx) ^ 0x80000000u;
	const auto     s = __builtin_amdgcn_permlane32_swap(a, b, false, false);
	float          t = fmin_num_f32(__uint_as_float(s[0]), __uint_as_float(s[1]));
	t                = fmin_num_f32(t, dpp_all_f32<0x121>(t));
	t                = fmin_num_f32(t, dpp_all_f32<0x122>(t));
	t                = fmin_num_f32(t, dpp_all_f32<0x124>(t));
	t                = fmin_num_f32(t, dpp_all_f32<0x128>(t));
	const int      r = static_cast<int>(__float_as_uint(t));
	t                = fmin_num_f32(t, __uint_as_float(static_cast<uint32_t>(__builtin_amdgcn_update_dpp(r, r, 0x142, 0xa, 0xf, false)))); // row_bcast:15 into rows 1 and 3
	const uint32_t u = __float_as_uint(t);
	mn               = __uint_as_float(__builtin_amdgcn_readlane(u, 31));
	mx               = __uint_as_float(__builtin_amdgcn_readlane(u, 63) ^ 0x80000000u);
}

// What a zone record ignores: a NaN, quiet or signalling, whatever its payload.  Kernels run in IEEE mode, where v_min / v_max skip a QUIET NaN
// operand but answer a signalling one with its quieted form, which would replace the accumulator.  v_max(x, x) is the canonicalisation: it
// quiets a signalling NaN and returns every other value, -0.0 included, as it is; the two instructions behind it then skip it.  Three vector
// instructions per value; mn and mx start as +inf / -inf and never become NaN.
__device__ __forceinline__ void minmax_take(double& mn, double& mx, double x) {
	const double q = fmax_num(x, x);
	mn             = fmin_num(mn, q);
	mx             = fmax_num(mx, q);
}
__device__ __forceinline__ void minmax_take(float& mn, float& mx, float x) {
	const float q = fmax_num_f32(x, x);
	mn            = fmin_num_f32(mn, q);
	mx            = fmax_num_f32(mx, q);
}

// ---- either precision -------------------------------------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void wave_minmax(T& mn, T& mx) {
	if constexpr (sizeof(T) == 8) { wave_minmax_f64(mn, mx); } else { wave_minmax_f32(mn, mx); }
}
template <class T>
__device__ __forceinline__ T pos_inf() {
	if constexpr (sizeof(T) == 8) { return __builtin_inf(); } else { return __builtin_inff(); }
}

// *addr = min(*addr, x) / max(*addr, x) in the records' order; x is not a NaN, *addr holds value bits
template <class T>
__device__ __forceinline__ void atomic_min_value(T* addr, T x) {
	if constexpr (sizeof(T) == 8) {
		const long long b = __double_as_longlong(x);
		if (b >= 0) { atomicMin(reinterpret_cast<long long*>(addr), b); } else { atomicMax(reinterpret_cast<unsigned long long*>(addr), static_cast<unsigned long long>(b)); }
	} else {
		const int b = static_cast<int>(__float_as_uint(x));
		if (b >= 0) { atomicMin(reinterpret_cast<int*>(addr), b); } else { atomicMax(reinterpret_cast<unsigned int*>(addr), static_cast<unsigned int>(b)); }
	}
}
template <class T>
__device__ __forceinline__ void atomic_max_value(T* addr, T x) {
	if constexpr (sizeof(T) == 8) {
		const long long b = __double_as_longlong(x);
		if (b >= 0) { atomicMax(reinterpret_cast<long long*>(addr), b); } else { atomicMin(reinterpret_cast<unsigned long long*>(addr), static_cast<unsigned long long>(b)); }
	} else {
		const int b = static_cast<int>(__float_as_uint(x));
		if (b >= 0) { atomicMax(reinterpret_cast<int*>(addr), b); } else { atomicMin(reinterpret_cast<unsigned int*>(addr), static_cast<unsigned int>(b)); }
	}
}

} // namespace alpgpu
