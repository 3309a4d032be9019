// gather_kernels.hip — random access into a compressed column: values by index (alpgpu_gather_*) and value slices (alpgpu_decode_slice_*).
//
// Value r of a column is value p = r & 1023 of vector v = r >> 10.  Its vector's descriptor gives the offsets, the width and the base; the
// FastLanes layout puts p at a known bit of a known word; the exception positions of a record ascend.  So one value costs a descriptor, one or
// two packed words (and for ALP_RD a left-index word and a dictionary entry) and a binary search of the positions — no vector is decoded
// whole.  One lane per output value, 256-thread workgroups; the value indices are loaded (gather) or are first + k (slice).  The arithmetic is
// the store decode's own (alp_device.hpp: decode_value, alp_device_f32.hpp: decode_value_f32, the same constant tables), so the bits are
// those alpgpu_decode_* writes at that index, exceptions patched in.
//
// Layouts (decode_kernels.hip / decode_f32_kernels.hip are the authority):
//   ALP double   u64 words, 16 lane streams x 64 rows: p -> lane p & 15, row p >> 4; stream word k of lane l at [16k + l]
//   ALP float    u32 words, 32 x 32: p -> lane p & 31, row p >> 5; word k of lane l at [32k + l]
//   ALP_RD       right parts as ALP at width rbw, base 0; left indices u16, 64 x 16 (p -> lane p & 63, row p >> 6) at packed_off + 128 rbw;
//                value bits = dict[index & 7] << rbw | right, where an exception replaces the dictionary entry by its left part
//   exceptions   ALP: cnt values (8 or 4 bytes) then cnt u16 positions; ALP_RD: cnt u16 left parts then cnt u16 positions
#include <type_traits>

#include "alp_device_f32.hpp"
#include "lane_field.hpp"
#include "launch.hpp"

namespace alpgpu {

constexpr int      kGatherThreads = 256;
constexpr uint64_t kGatherChunk   = 1ull << 31; // output values per launch (a grid holds fewer than 2^32 work-items)

// Rank of position p among the record's cnt ascending positions, or -1: a lower-bound search (at most 11 probes for 1024 positions).  The
// bound it ends on is always an element it probed (or cnt), so a probe that meets p is the hit and no load follows the search.
__device__ __forceinline__ int exception_rank(const uint16_t* __restrict__ pos, uint32_t cnt, uint32_t p) {
	uint32_t lo = 0, len = cnt;
	int      hit = -1;
	while (len > 0) {
		const uint32_t half = len >> 1;
		const uint32_t q    = pos[lo + half];
		hit                 = q == p ? static_cast<int>(lo + half) : hit;
		const bool less     = q < p;
		lo                  = less ? lo + half + 1 : lo;
		len                 = less ? len - half - 1 : half;
	}
	return hit;
}

// the bits alpgpu_decode_* writes for value p of vector v (VB = 8: double, 4: float)
template <int VB>
__device__ __forceinline__ uint64_t value_bits(const alpgpu_vector_desc* __restrict__ descs, const alpgpu_rowgroup_state* __restrict__ rgs,
                                               const uint8_t* __restrict__ packed, const uint8_t* __restrict__ excs, uint64_t v, uint32_t p) {
	typedef typename std::conditional<VB == 8, uint64_t, uint32_t>::type U;
	constexpr uint32_t       kLanes = VB == 8 ? 16u : 32u;
	const alpgpu_vector_desc d      = descs[v];
	const uint8_t*           rec    = excs + d.exc_off;
	const uint32_t           cnt    = d.exc_cnt;
	const U*                 words  = reinterpret_cast<const U*>(packed + d.packed_off);
	const U                  right  = lane_field<U, kLanes>(words + (p & (kLanes - 1)), p / kLanes, d.bw); // ALP: the digit; ALP_RD: the right part
	if (d.scheme == ALPGPU_SCHEME_ALP) {
		const int rank = cnt ? exception_rank(reinterpret_cast<const uint16_t*>(rec + static_cast<uint64_t>(VB) * cnt), cnt, p) : -1;
		if (rank >= 0) { return reinterpret_cast<const U*>(rec)[rank]; }
		if constexpr (VB == 8) {
			const uint32_t f = d.f < 18 ? d.f : 18, e = d.e < 20 ? d.e : 20; // (the tables' extents; a column that passes alpgpu_column_validate has e <= 18, f <= e)
			return static_cast<uint64_t>(__double_as_longlong(decode_value(static_cast<int64_t>(right + static_cast<uint64_t>(d.base)), kFactArr[f], kFracArr[e])));
		} else {
			const uint32_t f = d.f < 10 ? d.f : 10, e = d.e < 10 ? d.e : 10;
			return __float_as_uint(decode_value_f32(static_cast<int32_t>(right + static_cast<uint32_t>(d.base)), kFactArrF[f], kFracArrF[e]));
		}
	}
	// ALP_RD: the left index out of the u16 lanes behind the right parts, then the rowgroup's dictionary entry or the exception's left part
	const uint16_t* lefts = reinterpret_cast<const uint16_t*>(packed + d.packed_off + 128ull * d.bw);
	const uint32_t  idx   = lane_field<uint16_t, 64>(lefts + (p & 63u), p >> 6, d.lbw);
	const uint16_t  dict  = rgs[v / kRowgroup].rd_dict[idx & 7u];
	const int       rank  = cnt ? exception_rank(reinterpret_cast<const uint16_t*>(rec + 2ull * cnt), cnt, p) : -1;
	const U         left  = rank >= 0 ? reinterpret_cast<const uint16_t*>(rec)[rank] : dict;
	return static_cast<U>((left << d.bw) | right);
}

// LOADED: indices from d_idx (gather; out of range -> the canonical quiet NaN, nothing read), else first + k (slice; the host checked the range)
template <int VB, bool LOADED>
__global__ __launch_bounds__(kGatherThreads) void k_gather(const alpgpu_vector_desc* __restrict__ descs, const alpgpu_rowgroup_state* __restrict__ rgs,
                                                           const uint8_t* __restrict__ packed, const uint8_t* __restrict__ excs, const int64_t* __restrict__ d_idx,
                                                           uint64_t first, uint64_t k0, uint64_t n, uint64_t n_values, void* __restrict__ d_out) {
	typedef typename std::conditional<VB == 8, uint64_t, uint32_t>::type U;
	const uint64_t k = k0 + static_cast<uint64_t>(blockIdx.x) * kGatherThreads + threadIdx.x;
	if (k >= n) { return; }
	const uint64_t r    = LOADED ? static_cast<uint64_t>(d_idx[k]) : first + k;
	U              bits = VB == 8 ? static_cast<U>(0x7FF8000000000000ull) : static_cast<U>(0x7FC00000u); // (stored as an integer: no FP operation sees it)
	if (!LOADED || r < n_values) { bits = static_cast<U>(value_bits<VB>(descs, rgs, packed, excs, r >> 10, static_cast<uint32_t>(r & 1023u))); }
	reinterpret_cast<U*>(d_out)[k] = bits;
}

template <int VB, bool LOADED>
static void launch_gather_chunk(hipStream_t stream, const alpgpu_column* col, const int64_t* d_idx, uint64_t first, uint64_t k0, uint64_t n, void* d_out) {
	const uint64_t m = n - k0 < kGatherChunk ? n - k0 : kGatherChunk;
	hipLaunchKernelGGL((k_gather<VB, LOADED>), dim3(static_cast<unsigned>((m + kGatherThreads - 1) / kGatherThreads)), dim3(kGatherThreads), 0, stream, col->d_vectors,
	                   col->d_rowgroups, col->d_packed, col->d_exc, d_idx, first, k0, n, col->n_vectors * kVec, d_out);
}

int launch_gather(hipStream_t stream, const alpgpu_column* col, const int64_t* d_idx, uint64_t first, uint64_t n, void* d_out, int value_bytes) {
	for (uint64_t k0 = 0; k0 < n; k0 += kGatherChunk) {
		if (value_bytes == 8) {
			d_idx ? launch_gather_chunk<8, true>(stream, col, d_idx, first, k0, n, d_out) : launch_gather_chunk<8, false>(stream, col, d_idx, first, k0, n, d_out);
		} else {
			d_idx ? launch_gather_chunk<4, true>(stream, col, d_idx, first, k0, n, d_out) : launch_gather_chunk<4, false>(stream, col, d_idx, first, k0, n, d_out);
		}
		if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	}
	return ALPGPU_OK;
}

} // namespace alpgpu
