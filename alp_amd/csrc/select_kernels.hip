// select_kernels.hip — range selection on a compressed column (alpgpu_select_range_*): which value indices r of [first, first + n) hold a value x
// with lo <= x <= hi, in ascending order, and optionally those values.  The decoded column never reaches HBM.
//
// Three phases, ordered by kernel boundaries on one stream (no workgroup ever waits for another):
//   count  k_select<VB, kSelCount>  one wavefront per vector decodes it in registers and writes counts[v] = its number of qualifying values (u32)
//          k_select<VB, kSelCountZoned>  alpgpu_select_range_zoned_*: the same after a look at the vector's zone record {min, max}; a vector the record
//                               excludes, or admits whole, is counted from those 16 (8) bytes and its descriptor alone
//   scan   k_scan_*             exclusive prefix sum counts -> offsets (u64), blocks of 1024, block sums scanned the same way one level up;
//                               the top level writes *d_count
//   emit   k_select<VB, kSelEmit>  one wavefront per vector: counts[v] == 0 -> gone after a 4-byte read; else the same decode again, and every
//                               qualifying value's index (and value) goes to offsets[v] + its rank inside the vector, if below the capacity
//
// The decode of one vector by one wavefront is register_decode.hpp's (the layout of the steps, the exception mask, the arithmetic): step m holds
// value p = 64 m + lane in lane `lane`, so a wave-wide ballot of the predicate IS the 64 bits of the vector's qualify mask for indices 64 m ..
// 64 m + 63, in index order.  Rank inside the vector = qualifying values of the steps before (a wave-uniform running popcount) + the ballot's
// bits below the lane (v_mbcnt).  Ranks come from index-ordered masks and the offsets from a prefix sum, so the output ascends and is a function
// of the column and the arguments alone: no atomic decides a position.  A selected value has the bits alpgpu_decode_* writes at its index.
//
// HBM traffic: count reads every vector of the range once (descriptor, packed words, exception record, for ALP_RD the dictionary) and writes
// 4 bytes; the scan reads them and writes 8; emit reads 4 + 8 bytes per vector and, for vectors with a non-zero count only, the vector again,
// and writes 8 (+ 8 or 4) bytes per selected value.
//
// k_select, its one launcher (launch_select) and the scratch layout are in select_device.hpp, which mask_kernels.hip includes too (it launches three
// more arms of the kernel: the ballots kept as a bitmap, a masked SUM and a masked projection); this file holds the scan and the three phases.
#include "select_device.hpp"

namespace alpgpu {

// ---- the scan: out[i] = in[0] + ... + in[i - 1] --------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
	for (int s = 32; s > 0; s >>= 1) { x += __shfl_xor(x, s, 64); }
	return x;
}

// sums[b] = in[1024 b] + ... + in[1024 b + 1023]
template <class T>
__global__ __launch_bounds__(kScanBlock) void k_scan_reduce(const T* __restrict__ in, uint64_t n, uint64_t* __restrict__ sums) {
	__shared__ uint64_t s_wave[kScanBlock / 64];
	const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
	const uint64_t x = wave_sum(i < n ? static_cast<uint64_t>(in[i]) : 0ull);
	if ((threadIdx.x & 63u) == 0u) { s_wave[threadIdx.x >> 6] = x; }
	__syncthreads();
	if (threadIdx.x == 0) {
		uint64_t t = 0;
		for (int w = 0; w < kScanBlock / 64; ++w) { t += s_wave[w]; }
		sums[blockIdx.x] = t;
	}
}

// out[i] = block_off[b] + the sum of the block's elements before i (block_off == nullptr: one block, offset 0).  total (nullable): the sum of
// everything, written by the launch's last block — the caller passes it on the top level only.  in == out is allowed when T is uint64_t.
template <class T>
__global__ __launch_bounds__(kScanBlock) void k_scan_apply(const T* in, uint64_t n, const uint64_t* __restrict__ block_off, uint64_t* out, uint64_t* __restrict__ total) {
	__shared__ uint64_t s_wave[kScanBlock / 64];
	const uint64_t i    = static_cast<uint64_t>(blockIdx.x) * kScanBlock + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint64_t x    = i < n ? static_cast<uint64_t>(in[i]) : 0ull;
	uint64_t       incl = x;
	for (int s = 1; s < 64; s <<= 1) {
		const uint64_t y = __shfl_up(incl, s, 64);
		if (lane >= static_cast<uint32_t>(s)) { incl += y; }
	}
	if (lane == 63u) { s_wave[wave] = incl; }
	__syncthreads();
	uint64_t before = block_off ? block_off[blockIdx.x] : 0ull;
	for (uint32_t w = 0; w < wave; ++w) { before += s_wave[w]; }
	if (i < n) { out[i] = before + incl - x; }
	if (total != nullptr && blockIdx.x == gridDim.x - 1 && threadIdx.x == kScanBlock - 1) { *total = before + incl; }
}

static uint64_t scan_blocks(uint64_t n) { return (n + kScanBlock - 1) / kScanBlock; }

// Scratch of a select over a column of n_vectors: [offsets: u64 per vector][counts: u32 per vector][block sums of every scan level], each
// part rounded up to 16 bytes.  The levels shrink by 1024 each (n_vectors / 1024 + 1, that / 1024 + 1, ... down to one block: at most six
// for any n_vectors below 2^54), so the whole is at most 12 * n_vectors + n_vectors / 100 + 256 bytes.
uint64_t select_scratch_bytes(uint64_t n_vectors) {
	if (n_vectors > (1ull << 54)) { return ~0ull; }
	uint64_t bytes = align16(8ull * n_vectors) + align16(4ull * n_vectors);
	for (uint64_t len = n_vectors; len > kScanBlock;) {
		len = scan_blocks(len);
		bytes += align16(8ull * len);
	}
	return bytes < 16ull ? 16ull : bytes;
}

template <class T>
static int scan_level(hipStream_t stream, const T* in, uint64_t n, uint64_t* out, uint64_t* d_total, uint64_t* levels) {
	const uint64_t nb = scan_blocks(n);
	if (nb > 0x7FFFFFFFull) { return ALPGPU_ERR_INVALID; }
	if (nb <= 1) {
		hipLaunchKernelGGL((k_scan_apply<T>), dim3(1), dim3(kScanBlock), 0, stream, in, n, static_cast<const uint64_t*>(nullptr), out, d_total);
		return hipGetLastError() == hipSuccess ? ALPGPU_OK : ALPGPU_ERR_HIP;
	}
	hipLaunchKernelGGL((k_scan_reduce<T>), dim3(static_cast<unsigned>(nb)), dim3(kScanBlock), 0, stream, in, n, levels);
	if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	const int rc = scan_level<uint64_t>(stream, levels, nb, levels, d_total, levels + align16(8ull * nb) / 8ull); // the block sums, scanned in place one level up
	if (rc != ALPGPU_OK) { return rc; }
	hipLaunchKernelGGL((k_scan_apply<T>), dim3(static_cast<unsigned>(nb)), dim3(kScanBlock), 0, stream, in, n, static_cast<const uint64_t*>(levels), out,
	                   static_cast<uint64_t*>(nullptr));
	return hipGetLastError() == hipSuccess ? ALPGPU_OK : ALPGPU_ERR_HIP;
}

// d_offsets[i] = d_counts[0] + ... + d_counts[i - 1], *d_total = the sum of all n (n > 0); d_levels: the block-sum part of the scratch
int launch_select_scan(hipStream_t stream, const uint32_t* d_counts, uint64_t n, uint64_t* d_offsets, uint64_t* d_total, uint64_t* d_levels) {
	return scan_level<uint32_t>(stream, d_counts, n, d_offsets, d_total, d_levels);
}

// count (a.zones: the zone map, or null), scan, emit: `a` holds the count pass's arguments, the scratch's counts among them
template <int VB>
static int select_range(hipStream_t stream, const alpgpu_column* col, const SelArgs& a, const SelScratch& s, int64_t* d_idx, void* d_vals, uint64_t capacity, uint64_t* d_count) {
	int rc = a.zones != nullptr ? launch_select<VB, kSelCountZoned>(stream, col, a) : launch_select<VB, kSelCount>(stream, col, a);
	if (rc != ALPGPU_OK) { return rc; }
	rc = launch_select_scan(stream, s.counts, a.n_range, s.offsets, d_count, s.levels);
	if (rc != ALPGPU_OK || capacity == 0) { return rc; }
	SelArgs e  = a;
	e.zones    = nullptr;
	e.offsets  = s.offsets;
	e.d_idx    = d_idx;
	e.d_vals   = d_vals;
	e.capacity = capacity;
	return launch_select<VB, kSelEmit>(stream, col, e);
}

// n > 0 and first + n <= n_vectors * 1024 (the caller checked); d_scratch: select_scratch_bytes(col->n_vectors) bytes, 16-byte aligned
// d_zones (nullable): the column's zone map, one record per vector — the count pass then reads a vector's record before the vector
int launch_select_range(hipStream_t stream, const alpgpu_column* col, uint64_t first, uint64_t n, double lo, double hi, int64_t* d_idx, void* d_vals,
                        uint64_t capacity, uint64_t* d_count, void* d_scratch, int value_bytes, const void* d_zones) {
	const SelScratch s = select_scratch(d_scratch, col->n_vectors);
	SelArgs          a {};
	a.first   = first;
	a.end     = first + n;
	a.v0      = first >> 10;
	a.n_range = ((a.end - 1) >> 10) - a.v0 + 1;
	a.lo      = lo;
	a.hi      = hi;
	a.counts  = s.counts;
	a.zones   = d_zones;
	return value_bytes == 8 ? select_range<8>(stream, col, a, s, d_idx, d_vals, capacity, d_count) : select_range<4>(stream, col, a, s, d_idx, d_vals, capacity, d_count);
}

} // namespace alpgpu
