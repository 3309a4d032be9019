// exact_sum.hpp — the fixed-point representation of the exact keyed SUM (include/alpgpu.h, "exact keyed SUM": alpgpu_decode_keyed_exact_sum_*), host and
// device.  Plain integer code without HIP in it: keyed_sum_exact_kernels.hip includes it for its kernels, and a stand-alone host program can include it
// alone (tests/cpp/exact_sum_host.cpp does, under the sanitizers).
//
//   a finite double       +-m * 2^(p - 1074): m < 2^53 the significand (hidden bit included for normals), p = max(biased exponent, 1) - 1 in 0 .. 2045.
//   a key's table entry   kExactLimbs = 66 limbs of int64 and one word of flags.  Limb j has weight 2^(32 j - 1074).
//   a value               F = m << (p & 31) < 2^85, as three 32-bit chunks, is added to the limbs p >> 5, + 1 and + 2 (the highest is 65); each chunk
//                         negated for a negative value.  A limb therefore holds at most rows * (2^32 - 1) in magnitude: 2^31 rows never overflow one.
//   the flags             kExactNan, kExactPosInf, kExactNegInf: set for a NaN, +inf, -inf value, which reach no limb.
//   the result            exact_round_limbs: N = sum_j limb_j * 2^(32 j) times 2^-1074, rounded ONCE to nearest-even; +0.0 for N == 0; +-inf beyond
//                         DBL_MAX; the flags first (a NaN or both infinities: NaN; one infinity: that one).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ALPGPU_EXACT_HD __host__ __device__ inline
#else
#define ALPGPU_EXACT_HD inline
#endif

namespace alpgpu {

constexpr uint32_t kExactLimbs    = 66u;
constexpr uint32_t kExactKeyWords = kExactLimbs + 1u; // the table's stride per key, in 8-byte words: the limbs, then the flags
constexpr uint32_t kExactNan = 1u, kExactPosInf = 2u, kExactNegInf = 4u;

// What a value adds to its key's entry.  flags != 0: a NaN or an infinity, no chunk.  Otherwise chunk[k] (< 2^32) goes to limb + k, negated if negative;
// a zero (either sign) has three zero chunks.
struct ExactSplit {
	uint32_t flags;
	uint32_t negative;
	uint32_t limb; // 0 .. 63
	uint32_t chunk[3];
};

ALPGPU_EXACT_HD ExactSplit exact_split(uint64_t bits) {
	ExactSplit     s;
	const uint32_t e    = static_cast<uint32_t>(bits >> 52) & 0x7FFu;
	const uint64_t frac = bits & 0x000FFFFFFFFFFFFFull;
	s.negative          = static_cast<uint32_t>(bits >> 63);
	s.flags             = e != 0x7FFu ? 0u : frac != 0ull ? kExactNan : s.negative ? kExactNegInf : kExactPosInf;
	const uint64_t m    = e != 0u ? frac | 0x0010000000000000ull : frac;
	const uint32_t p    = (e != 0u ? e : 1u) - 1u;
	const uint32_t sh   = p & 31u;
	const uint64_t lo   = m << sh;                      // the low 64 bits of F
	const uint32_t hi   = static_cast<uint32_t>((m >> 32) >> (32u - sh)); // bits 64 .. 84 of F ((m >> 32) < 2^21: a 32-bit shift by 1 .. 32 in two steps)
	s.limb              = p >> 5;
	s.chunk[0]          = s.flags ? 0u : static_cast<uint32_t>(lo);
	s.chunk[1]          = s.flags ? 0u : static_cast<uint32_t>(lo >> 32);
	s.chunk[2]          = s.flags ? 0u : hi;
	return s;
}

// One pass over the limbs, low to high, as the digits (32 bits each) of sign * N; two more digits take the last carry in.  A limb plus a carry can pass
// 2^63, so a limb is split into its halves first: (low half + carry) has 34 bits, and the next carry is the high half plus that sum's.  Returns the last
// carry: 0, or -1 if sign * N is negative.  top: the index of the highest non-zero digit (-1: none); w[2] that digit, w[1] and w[0] the two below it,
// low: whether a digit below those is non-zero.
ALPGPU_EXACT_HD int64_t exact_digits(const int64_t* limbs, int64_t sign, int32_t& top, uint32_t (&w)[3], bool& low) {
	int64_t  carry = 0;
	uint32_t p1 = 0u, p2 = 0u; // the digits at j - 1 and j - 2
	bool     below = false;    // a non-zero digit under j - 2
	top = -1, w[0] = w[1] = w[2] = 0u, low = false;
	for (uint32_t j = 0; j < kExactLimbs + 2u; ++j) {
		const int64_t  limb = j < kExactLimbs ? sign * limbs[j] : 0; // (|limb| < 2^63: the negation is safe)
		const int64_t  s    = static_cast<int64_t>(static_cast<uint32_t>(limb)) + carry;
		const uint32_t d    = static_cast<uint32_t>(s);
		carry               = (limb >> 32) + (s >> 32); // (arithmetic shifts: floors)
		if (d != 0u) { top = static_cast<int32_t>(j), w[2] = d, w[1] = p1, w[0] = p2, low = below; }
		below = below || p2 != 0u;
		p2 = p1, p1 = d;
	}
	return carry;
}

// The rounded sum of a key's entry, as the bits of a double.
ALPGPU_EXACT_HD uint64_t exact_round_limbs_bits(const int64_t* limbs, uint64_t flags) {
	if ((flags & kExactNan) || ((flags & kExactPosInf) && (flags & kExactNegInf))) { return 0x7FF8000000000000ull; }
	if (flags & kExactPosInf) { return 0x7FF0000000000000ull; }
	if (flags & kExactNegInf) { return 0xFFF0000000000000ull; }
	int32_t  top;
	uint32_t w[3];
	bool     low;
	uint64_t sign = 0ull;
	if (exact_digits(limbs, 1, top, w, low) != 0) { // N < 0: the digits of -N
		sign = 0x8000000000000000ull;
		exact_digits(limbs, -1, top, w, low);
	}
	if (top < 0) { return 0ull; } // N == 0: +0.0
	const uint32_t b = 31u - static_cast<uint32_t>(__builtin_clz(w[2])); // the top bit within its digit
	const uint32_t P = 32u * static_cast<uint32_t>(top) + b;             // ... and within N: 2^P <= |N| < 2^(P + 1)
	const uint64_t hi64 = (static_cast<uint64_t>(w[2]) << 32) | w[1];
	if (P <= 52u) { return sign | (top == 0 ? static_cast<uint64_t>(w[2]) : hi64); } // |N| < 2^53 is its own bits: a subnormal, or the exponent field 1
	// |N|'s top 64 bits with the top bit at 63, and whether anything lies below them
	const uint32_t sh     = 31u - b;
	const uint64_t x      = sh != 0u ? (hi64 << sh) | (w[0] >> (32u - sh)) : hi64;
	const bool     sticky = (x & 0x3FFull) != 0ull || static_cast<uint32_t>(w[0] << sh) != 0u || low;
	uint64_t       mant   = x >> 11; // 53 bits
	if (((x >> 10) & 1ull) && (sticky || (mant & 1ull))) { ++mant; } // nearest, ties to even; 2^53 carries into the exponent below
	// |N| * 2^-1074 = mant * 2^(P - 52 - 1074): the exponent field is P - 51, and adding mant's hidden bit to the field below it writes it
	const uint64_t out = (static_cast<uint64_t>(P - 52u) << 52) + mant;
	return sign | (out < 0x7FF0000000000000ull ? out : 0x7FF0000000000000ull);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// host: the rounded sum as a double, and a value added to an entry (what the kernels do with integer atomics)
inline double exact_round_limbs(const int64_t (&limbs)[kExactLimbs], uint64_t flags) {
	const uint64_t b = exact_round_limbs_bits(limbs, flags);
	double         d;
	memcpy(&d, &b, sizeof d);
	return d;
}
inline void exact_add(int64_t (&limbs)[kExactLimbs], uint64_t& flags, double x) {
	uint64_t b;
	memcpy(&b, &x, sizeof b);
	const ExactSplit s = exact_split(b);
	flags |= s.flags;
	for (uint32_t k = 0; k < 3u; ++k) {
		if (s.chunk[k] != 0u) { limbs[s.limb + k] += s.negative ? -static_cast<int64_t>(s.chunk[k]) : static_cast<int64_t>(s.chunk[k]); }
	}
}
#endif

} // namespace alpgpu
