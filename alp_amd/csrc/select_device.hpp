// select_device.hpp — k_select<VB, ARM>, the kernel that every entry point of range selection and of the single-column bitmaps is an arm of, named by an
// integer constant and taking the column's streams and one record, SelArgs: shared by select_kernels.hip (kSelCount, kSelCountZoned, kSelEmit) and
// mask_kernels.hip (kSelMask: ballots kept as a bitmap, kSelSum: masked SUM, kSelTake: masked projection).  The decode of the vector is
// register_decode.hpp's, in batches of kSelBatch = 8 steps; what is here are the arms (their prologues and early exits, the predicate and the
// epilogues), the one launcher of them all (launch_select) and the layout of the caller's scratch.  Only those two files include this header for the
// kernel; join_kernels.hip includes it for the scratch's layout and the count-and-scan prologue (launch_mask_count_scan) that its bitmap route shares.
#pragma once
#include "register_decode.hpp"

namespace alpgpu {

constexpr int      kScanBlock = 1024; // counts per scan block = threads per scan workgroup
constexpr uint32_t kSelBatch  = 8;    // steps of a vector whose words are requested together
inline uint64_t    align16(uint64_t x) { return (x + 15ull) & ~15ull; } // the parts of the scratch (select_scratch_bytes) begin on 16 bytes

// the caller's scratch of a select over (or a bitmap of) n_vectors vectors: [offsets: u64 per vector][counts: u32 per vector][block sums of every scan level]
struct SelScratch {
	uint64_t* offsets;
	uint32_t* counts;
	uint64_t* levels;
};
// mask_kernels.hip: counts[v] = the set bits of vector v's 16 bitmap words, offsets = their exclusive prefix sum, *d_count = their total (n_vectors > 0)
int launch_mask_count_scan(hipStream_t stream, const uint64_t* d_mask, uint64_t n_vectors, uint64_t* d_count, const SelScratch& s);
inline SelScratch select_scratch(void* d_scratch, uint64_t n_vectors) {
	uint8_t* const base = static_cast<uint8_t*>(d_scratch);
	return SelScratch {reinterpret_cast<uint64_t*>(base), reinterpret_cast<uint32_t*>(base + align16(8ull * n_vectors)),
	                   reinterpret_cast<uint64_t*>(base + align16(8ull * n_vectors) + align16(4ull * n_vectors))};
}

// The arms.  [first, end) is the selected index range and [lo, hi] the closed value range of the four arms with a predicate; the launch covers vectors
// [v0, v0 + n_range), wavefront k of it vector v = v0 + k.
//   kSelCount       counts[k] = qualifying values of vector v; the launch covers exactly the vectors the range touches (v0 = first >> 10).
//   kSelCountZoned  the count pass of alpgpu_select_range_zoned_*: zones[v] = {min, max} (one record per vector of the COLUMN, indexed by v, not by k)
//                   is read first.  A vector whose zone misses [lo, hi] is counted 0 and one whose zone lies inside it, and which cannot hold a NaN,
//                   is counted whole; neither has its packed words or exception record read.
//   kSelEmit        the qualifying values' indices (and values) at offsets[k] + rank, under the capacity; counts[k] is the count pass's.
// The other three cover vectors of the whole column (mask_kernels.hip; include/alpgpu.h, "selection bitmaps") and word 16 v + m of the bitmap is step
// m's ballot: bit `lane` = value index 1024 v + 64 m + lane.
//   kSelMask        alpgpu_select_mask_*: the 16 ballots of a vector are not counted but kept, lane m < 16 holding step m's, combined with what the
//                   bitmap held (op) and stored as one run of 128 bytes.  A vector outside [first, end), one whose words are all zero under AND and
//                   one whose words are all ones under OR is settled from those 128 bytes: its descriptor is not read.
//   kSelSum         alpgpu_decode_sum_masked_*: no predicate; lane L adds the values 64 m + L whose bit is set, m ascending, from +0.0 (floats widened
//                   first), and the 64 partials combine by wave_tree_sum_f64.  A vector whose words are all zero gets +0.0 and 0 and is not read.
//   kSelTake        alpgpu_decode_masked_*: no predicate; the emit pass of a selection whose ballots are the bitmap's words.  counts[v] = the vector's
//                   set bits and offsets[v] = the set bits of the vectors before (k_mask_count and the scan ran first); the value at a set bit goes to
//                   d_vals (and its index to d_idx, nullable here) at offsets[v] + the set bits of the words before + those below the lane, under
//                   the capacity.  A vector with counts[v] == 0 costs those four bytes, one at or behind the capacity its offset too; a batch of
//                   kSelBatch steps whose words are all zero requests nothing of the column and only moves the exception rank on.
constexpr int kSelCount = 0, kSelCountZoned = 1, kSelEmit = 2, kSelMask = 3, kSelSum = 4, kSelTake = 5;
struct SelArgs { // an arm leaves the fields it does not read zero
	uint64_t        v0, n_range, wg_off; // every arm; this grid from workgroup wg_off on
	uint64_t        first, end;          // count, zoned count, emit, mask
	double          lo, hi;              // count, zoned count, emit, mask
	uint32_t*       counts;              // count, zoned count: written, [k]; emit: read, [k]
	const uint32_t* counts_in;           // take: [v], what k_mask_count wrote
	const uint64_t* offsets;             // emit: [k]; take: [v]
	int64_t*        d_idx;               // emit; take (nullable)
	void*           d_vals;              // emit (nullable); take
	uint64_t        capacity;            // emit, take
	uint64_t*       mask;                // mask: read and written
	const uint64_t* mask_in;             // sum, take
	int             op;                  // mask
	double*         sums;                // sum
	uint32_t*       sum_counts;          // sum (nullable)
	const void*     zones;               // zoned count
};
// One wavefront's vector, inlined into k_select below.  The four streams arrive as __restrict__ parameters and not as the fields of ColumnStreams:
// a function's parameters are where this compiler takes the promise that no store of the kernel reaches them (__restrict__ locals compile to the
// code of plain fields, byte for byte), and as plain fields the bitmap arms measured slower: profiles/r18_select_arms.txt.
template <int VB, int ARM>
__device__ __forceinline__ void select_vector(const alpgpu_vector_desc* __restrict__ descs, const alpgpu_rowgroup_state* __restrict__ rgs, const uint8_t* __restrict__ packed,
                                              const uint8_t* __restrict__ excs, const SelArgs& a) {
	const ColumnStreams c {descs, rgs, packed, excs};
	constexpr bool ZONED = ARM == kSelCountZoned, EMIT = ARM == kSelEmit, MASK = ARM == kSelMask, SUM = ARM == kSelSum, TAKE = ARM == kSelTake;
	typedef typename DecodeVec<VB>::U U;
	typedef typename DecodeVec<VB>::T T;
	__shared__ uint64_t s_exc[kSelWaves][16]; // per wavefront: bit p = value p is an exception

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t k    = (a.wg_off + blockIdx.x) * kSelWaves + wave;
	if (k >= a.n_range) { return; }
	const uint64_t v  = a.v0 + k;
	const uint64_t r0 = v << 10;
	uint32_t       p_begin, p_end; // (what they hold for a vector outside the range is not used: the MASK arm settles such a vector first)
	range_share(a.first, a.end, r0, p_begin, p_end);

	uint32_t total = 0;
	uint64_t out0  = 0;
	if constexpr (EMIT) {
		total = a.counts[k];
		if (total == 0) { return; } // a vector without a qualifying value costs these four bytes
		out0 = a.offsets[k];
		if (out0 >= a.capacity) { return; }
		if (a.d_vals == nullptr && total == p_end - p_begin) { // all of it qualifies and only indices are wanted: nothing to decode
			for (uint32_t p = p_begin + lane; p < p_end; p += 64u) {
				const uint64_t j = out0 + (p - p_begin);
				if (j < a.capacity) { a.d_idx[j] = static_cast<int64_t>(r0 + p); }
			}
			return;
		}
	}

	uint64_t prior = 0; // MASK, SUM, TAKE: lane m < 16 holds word m of the vector's bitmap as it was found
	if constexpr (MASK) {
		uint64_t* mw = a.mask + 16ull * v;
		// (written out in each of the three kernels that write a bitmap, and not a helper: the note at the end of register_decode.hpp)
		const bool outside = r0 >= a.end || r0 + 1024u <= a.first; // no value of the vector is in the range: q is false throughout
		if (a.op == kMaskSet) {
			if (outside) {
				if (lane < 16u) { mw[lane] = 0ull; }
				return;
			}
		} else {
			const uint64_t neutral = a.op == kMaskAnd ? 0ull : ~0ull; // the word that q cannot change
			prior                  = lane < 16u ? mw[lane] : neutral;
			if (ballot64(prior != neutral) == 0ull) { return; } // AND of all zeros, OR of all ones: these 128 bytes were all that was read
			if (outside) {
				if (a.op == kMaskAnd && lane < 16u) { mw[lane] = 0ull; }
				return;
			}
		}
	}
	if constexpr (SUM) {
		if (!bitmap_words(a.mask_in, v, lane, prior)) {
			if (lane == 0u) {
				a.sums[v] = 0.0;
				if (a.sum_counts != nullptr) { a.sum_counts[v] = 0u; }
			}
			return;
		}
	}

	if constexpr (TAKE) {
		total = a.counts_in[v];
		if (total == 0) { return; } // a vector without a set bit costs these four bytes
		out0 = a.offsets[v];
		if (out0 >= a.capacity) { return; } // ... and one at or behind the capacity these eight more: its descriptor is not read
		prior = lane < 16u ? a.mask_in[16ull * v + lane] : 0ull; // one read of 128 bytes
	}

	bool inside = false; // ZONED: every value the zone admits qualifies
	if constexpr (ZONED) {
		const T* zone = reinterpret_cast<const T*>(a.zones) + 2 * v; // (wave-uniform)
		const T  z_min = zone[0], z_max = zone[1];
		const T z_lo = static_cast<T>(a.lo), z_hi = static_cast<T>(a.hi);
		if (!(z_max >= z_lo && z_min <= z_hi)) { // excluded (a NaN bound excludes every vector): the record is all that was read
			if (lane == 0u) { a.counts[k] = 0u; }
			return;
		}
		inside = z_min >= z_lo && z_max <= z_hi;
	}
	const DecodeVec<VB> V = decode_vec_load<VB>(c, v);
	if constexpr (ZONED) {
		// contained: only a vector that cannot hold a NaN — ALP without exceptions (a NaN never round-trips through ALP, so it is always an exception)
		if (inside && V.alp && V.cnt == 0u) {
			if (lane == 0u) { a.counts[k] = p_end - p_begin; }
			return;
		}
	}
	const T lo = static_cast<T>(a.lo), hi = static_cast<T>(a.hi);
	exception_mask(V, s_exc, wave, lane);

	uint32_t before_exc = 0; // exceptions of the steps done
	uint32_t before_sel = 0; // qualifying values of the steps done (wave-uniform: it comes from ballots); SUM, TAKE: set bits of the steps done
	uint64_t keep       = 0; // MASK: lane m < 16 keeps step m's ballot
	double   acc        = 0.0; // SUM: this lane's partial
	for (uint32_t b = 0; b < 16u; b += kSelBatch) {
		if constexpr (TAKE) {
			// no bit set in these kSelBatch words: nothing of the column is requested, but the exceptions of the steps passed over still count
			// towards the rank of those behind them
			if (ballot64(lane >= b && lane < b + kSelBatch && prior != 0ull) == 0ull) {
				if (V.cnt > 0) {
#pragma unroll
					for (uint32_t i = 0; i < kSelBatch; ++i) { before_exc += static_cast<uint32_t>(__builtin_popcountll(s_exc[wave][b + i])); } // (every lane reads the same word)
				}
				continue;
			}
		}
		StepBatch<VB, kSelBatch> R;
		step_request(V, s_exc[wave], b, lane, before_exc, R);
#pragma unroll
		for (uint32_t i = 0; i < kSelBatch; ++i) {
			const uint32_t m    = b + i;
			const uint32_t p    = 64u * m + lane;
			const U        bits = step_bits(V, R, b, i, lane);
			const T        x    = value_of_bits<VB>(bits);
			if constexpr (SUM) {
				const uint64_t w = readlane64(prior, m);
				if ((w >> lane) & 1ull) { acc += static_cast<double>(x); } // (an addition alone: nothing to contract)
				before_sel += static_cast<uint32_t>(__builtin_popcountll(w));
				continue;
			}
			if constexpr (TAKE) {
				const uint64_t w = readlane64(prior, m);
				const uint64_t j = out0 + before_sel + mbcnt64(w, 0u);
				if (((w >> lane) & 1ull) && j < a.capacity) { // (lanes of a dense word store side by side)
					reinterpret_cast<U*>(a.d_vals)[j] = bits;
					if (a.d_idx != nullptr) { a.d_idx[j] = static_cast<int64_t>(r0 + p); }
				}
				before_sel += static_cast<uint32_t>(__builtin_popcountll(w));
				continue;
			}
			const bool     q   = p >= p_begin && p < p_end && x >= lo && x <= hi; // NaN (value or bound) never qualifies; -0.0 == 0.0
			const uint64_t sel = ballot64(q);
			if constexpr (MASK) { keep = lane == m ? sel : keep; }
			if constexpr (EMIT) {
				const uint64_t j = out0 + before_sel + mbcnt64(sel, 0u);
				if (q && j < a.capacity) {
					a.d_idx[j] = static_cast<int64_t>(r0 + p);
					if (a.d_vals != nullptr) { reinterpret_cast<U*>(a.d_vals)[j] = bits; }
				}
			}
			before_sel += static_cast<uint32_t>(__builtin_popcountll(sel));
		}
		if constexpr (EMIT || TAKE) {
			if (before_sel >= total || out0 + before_sel >= a.capacity) { return; } // the vector's last qualifying value, or the capacity, is behind us
		}
	}
	if constexpr (MASK) {
		if (lane < 16u) { a.mask[16ull * v + lane] = a.op == kMaskAnd ? (prior & keep) : a.op == kMaskOr ? (prior | keep) : keep; } // one run of 128 bytes
	} else if constexpr (SUM) {
		const double total_sum = wave_tree_sum_f64(acc);
		if (lane == 0u) {
			a.sums[v] = total_sum;
			if (a.sum_counts != nullptr) { a.sum_counts[v] = before_sel; }
		}
	} else if constexpr (!EMIT && !TAKE) {
		if (lane == 0u) { a.counts[k] = before_sel; }
	}
}
template <int VB, int ARM>
__global__ __launch_bounds__(kSelThreads) void k_select(const ColumnStreams c, const SelArgs a) {
	select_vector<VB, ARM>(c.descs, c.rgs, c.packed, c.excs, a);
}

// one pass of an arm over the a.n_range vectors from a.v0 on (host side), split only at the grid limit; static, as the launchers of the other kernels are
template <int VB, int ARM>
static int launch_select(hipStream_t stream, const alpgpu_column* col, SelArgs a) {
	const ColumnStreams c = column_streams(col);
	return launch_vectors(a.n_range, kSelWaves, [&](dim3 grid, uint64_t off) {
		a.wg_off = off;
		hipLaunchKernelGGL((k_select<VB, ARM>), grid, dim3(kSelThreads), 0, stream, c, a);
	});
}

} // namespace alpgpu
