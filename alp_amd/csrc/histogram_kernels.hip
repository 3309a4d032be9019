// histogram_kernels.hip — histograms (include/alpgpu.h, "histograms": alpgpu_histogram_*): the bucket counts of a compressed column's selected values by
// sorted edges.  It searches with lds_bound (sorted_list.hpp: the LDS tier of k_in_list's search) and counts as k_quantile_wide does (persistent_scan.hpp).
//
//   k_histogram<VB>   persistent workgroups of kHistWaves wavefronts.  The workgroup stages the edges into LDS and zeroes n_edges + 2 32-bit LDS bins,
//                     passes ONE workgroup barrier and then walks vectors v = wave id, wave id + waves, ...; every wavefront of a workgroup makes the
//                     same number of trips (the last may find no vector), so that the flush's barriers are met by all.  A vector is decoded in
//                     registers by register_decode.hpp in batches of kStepBatch steps, whose values search together, so that their LDS probes overlap.
//   the search        lds_bound: a branch-free bound over the edges [j0, j1), every step wave-uniform in its length: ceil(log2(j1 - j0 + 1)) probes; the result
//                     lies in [j0, j1] whatever the edges hold, and every probe index is clamped to the edges staged: an unsorted array gives
//                     unspecified buckets, reads nothing else and keeps the total.
//   the count         q_hist_add (quantile_device.hpp): one LDS add by the leading lane when a step's kept lanes agree on their bucket, otherwise one
//                     per kept lane; a step's selected NaNs are one add into bin n_edges + 1.
//   zones             a vector's record {min, max} (both no NaNs) is searched by the whole wavefront with the call's rule: j0 = bucket(min),
//                     j1 = bucket(max).  j0 == j1 and the descriptor says ALP without exceptions (only there a NaN is always an exception): the
//                     vector is the popcount of its selected bits into bin j0 and its packed words are not requested.  Any other vector is decoded
//                     with its per-value search over [j0, j1) only.  j1 < j0 (a record that lies) prunes nothing.
//   the flush         the workgroup's non-zero LDS bins into the 64-bit global counts by integer atomics, at the end and every flush_every trips
//                     (default kHistFlushEvery: a trip adds at most 8 x 1024 to one 32-bit bin).  No workgroup waits for another.
//
// HBM traffic per vector: the bitmap's 128 bytes (none with a NULL bitmap) and, unless they or the zone record settle the vector, its descriptor,
// packed words and exception record; the edges once per workgroup.  One launch of at most 3 workgroups per CU (what 49 KiB of LDS each allow).
//
// The few-bucket route (one ballot and popcount per admitted bucket and step into wave-uniform counters, for vectors that admit at most 8 buckets) is
// NOT in the library.  It was built and timed beside this kernel (profiles/r21_histogram.txt, second part): under 6 waves per SIMD the double kernel
// spilled (56 B of scratch) and the route won 2-5 % on the mixed and float columns at 8 buckets, lost 2-6 % on the ALP_RD column and 3-13 % in every
// cell of the zoned sorted column; without the cap it lost everywhere ("Histograms").  Word 2 of the trace stays 0.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; launch bounds 512 = 2 wavefronts per SIMD and workgroup;
// amdgpu_waves_per_eu(6): the 3 workgroups per CU that the LDS admits):
//   k_histogram<8>   78 VGPRs, 50192 B LDS, 6 waves per SIMD, no scratch (2 SGPRs kept in VGPR lanes)
//   k_histogram<4>   68 VGPRs, 33808 B LDS, 7 waves per SIMD, no scratch
// (The float kernel's LDS would admit a fourth workgroup per CU, its registers not the eighth wavefront per SIMD that takes: three for both.)
#include "persistent_scan.hpp"
#include "quantile_device.hpp"
#include "sorted_list.hpp"

namespace alpgpu {

constexpr int      kHistWaves      = 8; // wavefronts per workgroup: they share the staged edges and the bins
constexpr int      kHistThreads    = 64 * kHistWaves;
constexpr int      kHistWgPerCu    = 3;        // 49 KiB of LDS each (double; 33 KiB for float, the same grid)
constexpr uint32_t kHistEdgeWords  = ALPGPU_HISTOGRAM_EDGES_MAX + 1u; // LDS words of edges
constexpr uint32_t kHistBinWords   = ALPGPU_HISTOGRAM_EDGES_MAX + 2u; // LDS bins: n_edges + 1 buckets and the NaN counter
constexpr uint32_t kHistFlushEvery = 1u << 18; // trips of a workgroup's loop (8 vectors each, at most 8192 increments of one 32-bit LDS bin) between two flushes

struct HistArgs {
	uint64_t        n_vectors;
	uint64_t        first, end; // the selected index range
	const uint64_t* mask;       // nullable: every value of the range
	const void*     edges;      // n_edges sorted elements of the column's type
	const void*     zones;      // nullable: one record {min, max} per vector
	uint64_t*       counts;     // n_edges + 2 words, added to
	uint64_t*       trace;      // nullable: 4 words, added to
	uint32_t        n_edges;    // <= ALPGPU_HISTOGRAM_EDGES_MAX
	uint32_t        right;      // 0: bucket = #{e <= x}, else #{e < x}
	uint32_t        flush_every;
};

// out[i] = j0 + the edges e of [j0, j1) with e <= x[i] (right: e < x[i]); a NaN edge is never <= anything: inert.  No edges: j0 == j1, nothing is read.
template <int VB, uint32_t NB>
__device__ __forceinline__ void hist_buckets(const typename DecodeVec<VB>::T* s_edges, const HistArgs& g, uint32_t j0, uint32_t j1, const typename DecodeVec<VB>::T (&x)[NB],
                                             uint32_t (&out)[NB]) {
	lds_bound<typename DecodeVec<VB>::T, NB>(s_edges, g.n_edges > 0u ? g.n_edges - 1u : 0u, j0, j1, x, g.right != 0u ? 0u : ~0u, out);
}

constexpr uint32_t kHistSkipZero = 0u, kHistZone = 1u, kHistFew = 2u, kHistDecoded = 3u; // what hist_vector did with a vector: the trace's words

// One vector by one wavefront.  Returns the class of the trace it fell into.
template <int VB>
__device__ __forceinline__ uint32_t hist_vector(const ColumnStreams& c, const HistArgs& g, uint64_t v, uint32_t wave, uint32_t lane, const typename DecodeVec<VB>::T* s_edges,
                                                uint32_t* s_bins, uint64_t (&s_exc)[kHistWaves][16]) {
	typedef typename DecodeVec<VB>::T T;
	// 1. the selected bits: the vector's 128 bytes of bitmap (all ones without one), lane m < 16 holding word m, ANDed with the range's share
	const uint64_t r0 = v << 10;
	if (r0 >= g.end || r0 + 1024u <= g.first) { return kHistSkipZero; } // no value of the vector is in the range: nothing is read
	uint64_t sel;
	if (!selected_words(g.mask, g.first, g.end, v, lane, sel)) { return kHistSkipZero; }

	// 2. the part [j0, j1) of the edges that the vector's zone record admits: all of them without a record, with a NaN bound or with min above max
	uint32_t j0 = 0u, j1 = g.n_edges;
	if (g.zones != nullptr) {
		const T* zone = static_cast<const T*>(g.zones) + 2 * v; // (wave-uniform)
		const T  z[2] = {zone[0], zone[1]};
		if (z[0] == z[0] && z[1] == z[1]) {
			uint32_t j[2];
			hist_buckets<VB, 2>(s_edges, g, 0u, g.n_edges, z, j); // the buckets of min and of max
			const uint32_t a = __builtin_amdgcn_readfirstlane(j[0]), b = __builtin_amdgcn_readfirstlane(j[1]);
			if (a <= b) {
				j0 = a;
				j1 = b;
				if (j0 == j1) {
					if (alp_without_exceptions(c.descs[v])) { // no NaN can hide here: the selected bits are the count of bucket j0
						const uint32_t n = selected_count(sel);
						if (lane == 63u) { atomicAdd(&s_bins[j0], n); }
						return kHistZone;
					}
				}
			}
		}
	}

	// 3. the descriptor, the dictionary and the exception mask
	const DecodeVec<VB> V = decode_vec_load<VB>(c, v);
	exception_mask(V, s_exc, wave, lane);

	uint32_t before_exc = 0; // exceptions of the steps done
	for (uint32_t b = 0; b < 16u; b += kStepBatch) {
		// 4. every load of kStepBatch steps is requested before the first is used
		StepBatch<VB, kStepBatch> R;
		step_request(V, s_exc[wave], b, lane, before_exc, R);
		T x[kStepBatch];
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) { x[i] = step_value(V, R, b, i, lane); }
		// 5. the batch's buckets, searched together
		uint32_t at[kStepBatch];
		hist_buckets<VB, kStepBatch>(s_edges, g, j0, j1, x, at);
		// 6. per step: the selected values that are no NaNs into their buckets, the selected NaNs into the last bin
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			const uint64_t w    = readlane64(sel, b + i);
			const uint64_t nans = ballot64(top_k_is_nan<VB>(x[i]));
			q_hist_add(s_bins, w & ~nans, at[i], lane);
			if ((w & nans) != 0ull && lane == 0u) { atomicAdd(&s_bins[g.n_edges + 1u], static_cast<uint32_t>(__builtin_popcountll(w & nans))); }
		}
	}
	return kHistDecoded;
}

// (6 wavefronts per SIMD are 3 workgroups per CU, what their LDS admits: the compiler is held to the 80 registers that takes)
template <int VB>
__global__ __launch_bounds__(kHistThreads) __attribute__((amdgpu_waves_per_eu(6))) void k_histogram(const ColumnStreams c, const HistArgs g) {
	typedef typename DecodeVec<VB>::T T;
	__shared__ T        s_edges[kHistEdgeWords];
	__shared__ uint32_t s_bins[kHistBinWords];
	__shared__ uint64_t s_exc[kHistWaves][16]; // per wavefront: bit p = value p is an exception

	const uint32_t wave   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane   = threadIdx.x & 63u;
	const uint32_t n_bins = g.n_edges + 2u;

	// 0. the edges into LDS and the bins zeroed, once per workgroup; the one barrier in front of the loop
	const T* edges = static_cast<const T*>(g.edges);
	for (uint32_t i = threadIdx.x; i < g.n_edges; i += kHistThreads) { s_edges[i] = edges[i]; }
	bins_zero<kHistThreads>(s_bins, n_bins);
	__syncthreads();

	// every wavefront of the workgroup makes the same number of trips (the last may find no vector), so that the flush's barriers are met by all
	const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * kHistWaves;
	uint32_t       did[4]  = {0u, 0u, 0u, 0u};
	uint32_t       trips   = 0;
	for (uint64_t k0 = static_cast<uint64_t>(blockIdx.x) * kHistWaves; k0 < g.n_vectors; k0 += n_waves) {
		const uint64_t v = k0 + wave;
		if (v < g.n_vectors) {
			const uint32_t what = hist_vector<VB>(c, g, v, wave, lane, s_edges, s_bins, s_exc);
#pragma unroll
			for (uint32_t i = 0; i < 4u; ++i) { did[i] += what == i ? 1u : 0u; }
		}
		if (++trips == g.flush_every) {
			trips = 0;
			bins_flush<kHistThreads>(s_bins, n_bins, g.counts);
			__syncthreads();
			bins_zero<kHistThreads>(s_bins, n_bins);
			__syncthreads();
		}
	}
	bins_flush<kHistThreads>(s_bins, n_bins, g.counts);
	if (g.trace != nullptr && lane < 4u) { // the trace: one add per wavefront and counter
		const uint32_t mine = lane == 0u ? did[0] : lane == 1u ? did[1] : lane == 2u ? did[2] : did[3];
		if (mine != 0u) { atomicAdd(reinterpret_cast<unsigned long long*>(g.trace) + lane, static_cast<unsigned long long>(mine)); }
	}
}

// col->n_vectors > 0, n > 0, n_edges <= ALPGPU_HISTOGRAM_EDGES_MAX; range and alignments checked by the caller; the counts are added to
// (a call that overwrites has zeroed them by launch_fill_u64: mask_kernels.hip says why that is a kernel and no memset node)
int launch_histogram(hipStream_t stream, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const void* d_zones, const void* d_edges, uint32_t n_edges,
                     int right, uint64_t* d_counts, int value_bytes, int n_cus, const alpgpu_histogram_tuning* tuning, uint64_t* d_trace) {
	HistArgs args {};
	args.n_vectors   = col->n_vectors;
	args.first       = first;
	args.end         = first + n;
	args.mask        = d_mask;
	args.edges       = d_edges;
	args.zones       = d_zones;
	args.counts      = d_counts;
	args.trace       = d_trace;
	args.n_edges     = n_edges;
	args.right       = right != 0;
	args.flush_every = tuning != nullptr && tuning->flush_every != 0u && tuning->flush_every < kHistFlushEvery ? tuning->flush_every : kHistFlushEvery;
	// sized to the device: a workgroup stages the edges once
	const unsigned grid = persistent_grid(col->n_vectors, kHistWaves, n_cus, kHistWgPerCu, 0, tuning != nullptr ? tuning->grid : 0u, kTuningGridMax);
	const ColumnStreams c = column_streams(col);
	if (value_bytes == 8) {
		hipLaunchKernelGGL((k_histogram<8>), dim3(grid), dim3(kHistThreads), 0, stream, c, args);
	} else {
		hipLaunchKernelGGL((k_histogram<4>), dim3(grid), dim3(kHistThreads), 0, stream, c, args);
	}
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

} // namespace alpgpu
