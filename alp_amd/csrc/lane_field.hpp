// lane_field.hpp — one field of a FastLanes lane stream, read where it lies: what the random-access kernels (gather_kernels.hip) and the selection
// kernels (select_kernels.hip) unpack with.  The layouts are described in gather_kernels.hip.
#pragma once
#include <stdint.h>

#include <type_traits>

namespace alpgpu {

// Field `row` (width bw) of a FastLanes lane stream of U words that lie STRIDE words apart from w on.  The second word is read only if the
// field reaches into it: nothing past the vector's words is read.
template <class U, int STRIDE>
__device__ __forceinline__ U lane_field(const U* __restrict__ w, uint32_t row, uint32_t bw) {
	typedef typename std::conditional<sizeof(U) == 8, uint64_t, uint32_t>::type C; // (u16 lanes are computed in 32 bits)
	constexpr uint32_t kBits = 8 * sizeof(U);
	if (bw == 0) { return 0; }
	const uint32_t bit = row * bw;
	const uint32_t s   = bit & (kBits - 1);
	const U*       at  = w + STRIDE * (bit / kBits);
	const C        lo  = at[0];
	const C        hi  = s + bw > kBits ? C(at[STRIDE]) : C(0);
	const C        msk = bw >= kBits ? C(static_cast<U>(~U(0))) : ((C(1) << bw) - C(1));
	return static_cast<U>(((lo >> s) | ((hi << 1) << (kBits - 1 - s))) & msk); // (hi << (kBits - s)) without the undefined shift by kBits when s == 0
}

// The same field in two halves, for a caller that wants the loads of several fields in flight before it uses the first (select_kernels.hip): both
// words are always loaded — a field that does not reach into a second word loads its first word twice, so nothing past the vector's words is read
// and no branch stands between the loads — and what the repeated word shifts in lies above the field, where the mask removes it.  bw > 0.
template <class U>
struct FieldWords {
	typename std::conditional<sizeof(U) == 8, uint64_t, uint32_t>::type lo, hi;
};
template <class U, int STRIDE>
__device__ __forceinline__ FieldWords<U> load_field_words(const U* __restrict__ w, uint32_t row, uint32_t bw) {
	constexpr uint32_t kBits = 8 * sizeof(U);
	const uint32_t     bit   = row * bw;
	const U*           at    = w + STRIDE * (bit / kBits);
	return FieldWords<U> {at[0], at[(bit & (kBits - 1)) + bw > kBits ? STRIDE : 0]};
}
template <class U>
__device__ __forceinline__ U extract_field(const FieldWords<U>& f, uint32_t row, uint32_t bw) {
	typedef typename std::conditional<sizeof(U) == 8, uint64_t, uint32_t>::type C;
	constexpr uint32_t kBits = 8 * sizeof(U);
	const uint32_t     s     = (row * bw) & (kBits - 1);
	const C            msk   = bw >= kBits ? C(static_cast<U>(~U(0))) : ((C(1) << bw) - C(1));
	return static_cast<U>(((f.lo >> s) | ((f.hi << 1) << (kBits - 1 - s))) & msk);
}

} // namespace alpgpu
