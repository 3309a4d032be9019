// staged_decode.hpp — what the store decode and its sinks share across the two precisions (decode_kernels.hip, decode_f32_kernels.hip; the mask and the
// buffer resources also consume_kernels.hip and decode_stream_f32_kernels.hip): everything around the unpack.  The unpack itself differs — pairs of 64-bit
// fields in decode_vector_quarters, quads of 32-bit fields in finish_quad_f32 — and stays with its kernel.  VB is the value width in bytes (8 or 4); LDS is
// the record a workgroup (DecodeLdsT, DecodeLdsF32) or a wavefront (SinkWaveLds, SinkWaveLdsF32) stages one vector in:
//   stage[], kStage   the packed words as they lie in the stream, + the unit row past the end that the unpack reads and masks off
//   mask[32]          the exception positions as 1024 bits
//   excv[], kExcBytes the head of the exception record (its values come first), brought in by LDS-DMA
//   rdict[8]          ALP_RD: the rowgroup's dictionary
//   pref[32]          (kPrefixInLds, the one-wavefront sinks) exceptions in front of mask word i
#pragma once
#include "alp_device.hpp"

namespace alpgpu {

constexpr int kDecWaves   = 4; // wavefronts cooperating on one vector
constexpr int kDecThreads = 64 * kDecWaves;

// The exception mask (32 words) as seen by one wavefront: lane l < 32 holds word l and the number of exceptions in the
// words before it.  The prefix is a DPP row scan (register-to-register; a __shfl_up chain would be five dependent trips
// through the LDS crossbar on the critical path of a latency-bound workgroup), the per-step lookups below are readlanes.
struct ExcMask {
	uint32_t word; // mask word (lane & 31)
	int      excl; // exceptions in words 0 .. (lane & 31) - 1
};
template <class LDS>
__device__ __forceinline__ ExcMask load_exception_mask(const LDS& L, int lane) {
	ExcMask   m;
	m.word  = L.mask[lane & 31];
	const int c = lane < 32 ? __builtin_popcount(m.word) : 0;
	int       v = c;
	v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false); // row_shr:1
	v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false); // row_shr:2
	v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false); // row_shr:4
	v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false); // row_shr:8   -> inclusive scan inside each 16-lane row
	v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false); // row_bcast:15 -> row 1 += total of row 0 (lanes 0..31 done)
	m.excl = v - c;
	return m;
}

// the value of the exception of that rank: staged (LDS) or, past the stage, from HBM.  all_staged (wave-uniform: the vector's count fits the
// stage) keeps the common case to the LDS read alone — written as "LDS if rank < kStaged else HBM" the compiler selects between the two
// ADDRESSES and issues ONE FLAT load per exception (v_cndmask on pointers, src_shared_base): slower than either, and it waits for every counter.
// (cured in the double kernel in round 3, found again in the float sink's ISA in round 5: profiles/r05_float_sink.txt)
template <int VAL_BYTES, class REG = std::conditional_t<VAL_BYTES == 8, uint64_t, uint32_t>, class LDS>
__device__ __forceinline__ REG fetch_exception(const LDS& L, const uint8_t* __restrict__ rec, int rank, bool all_staged) {
	typedef std::conditional_t<VAL_BYTES == 8, uint64_t, std::conditional_t<VAL_BYTES == 4, uint32_t, uint16_t>> stored_t;
	constexpr int kStaged = static_cast<int>(LDS::kExcBytes) / VAL_BYTES;
	const int     at      = rank < kStaged ? rank : kStaged - 1;
	REG           v       = reinterpret_cast<const stored_t*>(L.excv)[at];
	if constexpr (LDS::kPrefixInLds) {
		asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v)::"memory"); // (k_sink_direct: as in exception_hits_lds) ... and keeps the two loads two loads
	} else {
		asm volatile("" : "+v"(v)); // keeps the two loads two loads
	}
	if (!all_staged) {
		if (rank >= kStaged) { v = reinterpret_cast<const stored_t*>(rec)[rank]; }
	}
	return v;
}

// exception lookup for the pair (128*m + 2*lane, +1): 2-bit hit mask and the rank of the first hit.  m is wave-uniform.  The pair's mask
// word is 4m + (lane >> 4): word and prefix come from the lane that holds them by ds_bpermute (the LDS crossbar, no memory) — as eight
// readlanes and six selects per step this lookup was a quarter of the vector instructions of a vector with exceptions, and the consumers
// (SUM / COUNT sinks) are bound by exactly those (profiles/r03_consumers.txt).
// The same lookup out of the wavefront's LDS (mask word and its prefix as two ds_read_b32 of one address per 16 lanes) — what k_sink_direct
// uses.  SOME BUILDS of that kernel (another register budget, another batch size, two compiler pins ...) come back with a wrong extracted
// field in the step FOLLOWING an exception lookup — right words in the registers, wrong value — for ~5 % of the exception-carrying
// vectors of a long column, never the same ones; a build either does it in every run or never.  Three such builds became clean with this
// form instead of ds_bpermute; later one with this form was wrong again, clean with full LDS waits, and another wrong WITH them.  None of
// that was the cause: the wrong builds had a 64-bit shift's amount in the LAST register of their allocation, which gfx950 reads as VGPR0
// there (see k_sink_direct; profiles/r03_consumers.txt has the way to it).  The LDS form stayed (same speed).  A build of decode_kernels.hip
// ships only if tools/check_top_vgpr.py is clean and tests/test_decode_sum_gpu.py::test_exception_records_that_change_nothing and
// ...across_a_full_chip pass.  k_decode_column uses 44 of 48 allocated registers: the pattern cannot arise there.
template <class LDS>
__device__ __forceinline__ uint32_t exception_hits_lds(const LDS& L, int m, int lane, int& rank) {
	const int      q    = 4 * m + (lane >> 4);
	uint32_t       word = L.mask[q];
	int            pref = static_cast<int>(L.pref[q]);
	asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(word), "+v"(pref)::"memory"); // both words here before anything is computed from them (see above: not a cure by itself)
	const int      b0   = (2 * lane) & 31;
	const uint32_t hits = (word >> b0) & 3u;
	rank                = pref + __builtin_popcount(word & ((1u << b0) - 1u));
	return hits;
}
__device__ __forceinline__ uint32_t exception_hits(const ExcMask& em, int m, int lane, int& rank) {
	const int      src  = (4 * m + (lane >> 4)) << 2; // byte address of the source lane
	const uint32_t word = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(src, static_cast<int>(em.word)));
	const int      pref = __builtin_amdgcn_ds_bpermute(src, em.excl);
	const int      b0   = (2 * lane) & 31;
	const uint32_t hits = (word >> b0) & 3u;
	rank                = pref + __builtin_popcount(word & ((1u << b0) - 1u));
	return hits;
}

// ALP_RD (is_rd, wave-uniform): the rowgroup's dictionary (RdDict's two words: 8 x u16) into the vector's LDS, by the first four lanes of the caller's group
template <class LDS, class CONSTS>
__device__ __forceinline__ void stage_rd_dictionary(LDS& L, const CONSTS& dict, int tid) {
	{ reinterpret_cast<uint32_t*>(L.rdict)[tid] = static_cast<uint32_t>((tid < 2 ? dict.lo : dict.hi) >> (32 * (tid & 1))); }
}

// HBM through buffer loads: two resources sized to the vector's packed words (right words; ALP_RD: the left words behind them), so reads past its last
// unit / last left word return 0 (what the unpack reads there is masked off anyway) without a clamp per load
// (W: the widths as the caller holds them, descriptor bytes or ints — converted here, the scalar prologue of the one-wavefront sinks comes out differently)
template <class WORDS, class W>
__device__ __forceinline__ WORDS packed_word_resources(const uint8_t* packed_words, W bw, W lbw, bool is_alp) {
	uint8_t*      first      = const_cast<uint8_t*>(packed_words);
	constexpr int kRsrcFlags = 0x00020000; // gfx9 raw buffer, 32-bit data format
	return WORDS {__builtin_amdgcn_make_buffer_rsrc(first, 0, 128 * bw, kRsrcFlags), __builtin_amdgcn_make_buffer_rsrc(first + 128u * bw, 0, is_alp ? 0 : 128 * lbw, kRsrcFlags)};
}

// Issues every load of one vector: packed words and the values of its exceptions straight into LDS (global_load_lds, 16 resp. 4 bytes per
// lane, no VGPR round trip), exception positions into registers.  (Until round 3 the values went through registers too, behind a branch on the
// scheme for their width — and the compiler's wait-count pass put an s_waitcnt vmcnt(0) between the two arms, i.e. a whole HBM round trip in
// front of the packed loads of every vector with exceptions of one of the two schemes.)
// (a double vector whose words do not fit the workgroup's stage — a malformed descriptor: every well-formed vector of either precision fits — is not staged.  The
// float kernels never had the test and stay without it: with it their scalar prologue grows by four instructions per vector, which was not timed.)
template <class LDS>
__device__ __forceinline__ bool vector_fits_stage(const alpgpu_vector_desc& d) {
	return 128 * (static_cast<int>(d.bw) + (d.scheme == ALPGPU_SCHEME_ALP ? 0 : static_cast<int>(d.lbw))) + 128 <= LDS::kStage;
}
template <int VB, class LDS>
__device__ __forceinline__ uint32_t issue_vector_loads(LDS& L, const alpgpu_vector_desc& d, const uint8_t* __restrict__ packed,
                                                       const uint8_t* __restrict__ rec, int tid, int wave) {
	typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
	constexpr int T       = kDecThreads;
	const bool    is_alp  = d.scheme == ALPGPU_SCHEME_ALP;
	const int     n_units = (VB == 4 || vector_fits_stage<LDS>(d)) ? 8 * (d.bw + (is_alp ? 0 : d.lbw)) : 0;
	const ull2*   g       = reinterpret_cast<const ull2*>(packed + d.packed_off);
	constexpr int kWidest   = 8 * (8 * VB + 2); // units of the widest vector: ALP_RD, 8 VB - 1 right and 3 left bits
	constexpr int kMaxUnits = (LDS::kStage - 128) / 16 < kWidest ? (LDS::kStage - 128) / 16 : kWidest;
#pragma unroll
	for (int j = 0; j < (kMaxUnits + T - 1) / T; ++j) {
		const int c = tid + T * j;
		if (c < n_units) { // LDS destination = wave-uniform base + 16 * lane
			__builtin_amdgcn_global_load_lds(g + c, reinterpret_cast<ull2*>(L.stage) + (T * j + 64 * wave), 16, 0, 0);
		}
	}
	uint32_t  pos = 0u;
	const int cnt = d.exc_cnt;
	if (cnt > 0) { // wave-uniform
		const uint32_t val_bytes = (is_alp ? static_cast<uint32_t>(VB) : 2u) * static_cast<uint32_t>(cnt);
		const int      dwords    = static_cast<int>(((val_bytes < LDS::kExcBytes ? val_bytes : LDS::kExcBytes) + 3u) >> 2); // (records are 8-byte multiples)
		static_assert(LDS::kExcBytes / 4 <= 2 * T, "two loads per thread cover the stage");
		if (tid < dwords) { __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint32_t*>(rec) + tid, reinterpret_cast<uint32_t*>(L.excv) + 64 * wave, 4, 0, 0); }
		if constexpr (LDS::kExcBytes / 4 > T) {
			if (tid + T < dwords) { __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint32_t*>(rec) + T + tid, reinterpret_cast<uint32_t*>(L.excv) + T + 64 * wave, 4, 0, 0); }
		}
		if (tid < cnt) { pos = reinterpret_cast<const uint16_t*>(rec + val_bytes)[tid]; }
	}
	return pos;
}

template <int VB, class LDS>
__device__ __forceinline__ void land_exceptions(LDS& L, const alpgpu_vector_desc& d, const uint8_t* __restrict__ rec, uint32_t pos, int tid) {
	constexpr int T   = kDecThreads;
	const int     cnt = d.exc_cnt;
	if (tid < cnt) { atomicOr(&L.mask[pos >> 5], 1u << (pos & 31)); }
	if (cnt > T) { // more exceptions than threads in one vector: rare
		const uint16_t* poss = reinterpret_cast<const uint16_t*>(rec + static_cast<size_t>(cnt) * (d.scheme == ALPGPU_SCHEME_ALP ? VB : 2));
		for (int j = tid + T; j < cnt; j += T) {
			const uint32_t p = poss[j];
			atomicOr(&L.mask[p >> 5], 1u << (p & 31));
		}
	}
}

// ---- the workgroup kernels (k_decode_column, k_decode_column_f32): V consecutive vectors per 256-thread workgroup -------------------------------------
// From the descriptor loads to the barrier behind which d[], dict[] and the staged L[] are whole: all loads of all V vectors are in flight together.
// load_consts(v, d) = the per-vector constants of vector v (their table reads depend on the descriptor alone and are in flight with the packed words).
template <int VB, int V, class LDS, class CONSTS, class LOAD_CONSTS>
__device__ __forceinline__ void stage_vectors(LDS (&L)[V], alpgpu_vector_desc (&d)[V], CONSTS (&dict)[V], const alpgpu_vector_desc* descs,
                                              const uint8_t* packed, const uint8_t* excs, uint64_t v0, uint64_t n_vectors, int tid, int wave,
                                              LOAD_CONSTS load_consts) {
	uint32_t pos[V];
#pragma unroll
	for (int i = 0; i < V; ++i) {
		const uint64_t v = v0 + i < n_vectors ? v0 + i : v0; // the odd tail vector is simply loaded twice
		d[i]             = descs[v];
	}
#pragma unroll
	for (int i = 0; i < V; ++i) { dict[i] = load_consts(v0 + i < n_vectors ? v0 + i : v0, d[i]); }
#pragma unroll
	for (int i = 0; i < V; ++i) { pos[i] = issue_vector_loads<VB>(L[i], d[i], packed, excs + d[i].exc_off, tid, wave); }
	// ALP_RD vectors: the dictionary into the vector's LDS (four lanes; visible behind the barrier below)
#pragma unroll
	for (int i = 0; i < V; ++i) {
		if (d[i].scheme != ALPGPU_SCHEME_ALP && tid < 4) { stage_rd_dictionary(L[i], dict[i], tid); }
	}
	// Only a workgroup that has exceptions zeroes its masks, and it does so behind the issue of all its loads: the barrier that fences the
	// zeroes from the atomics waits for LDS only, so it falls into the shadow of the HBM round trip.  (Until round 3 every workgroup,
	// exceptions or not, began with the zeroing write and a barrier in front of its first load.)
	bool any_exc = false;
#pragma unroll
	for (int i = 0; i < V; ++i) { any_exc |= d[i].exc_cnt != 0; }
	if (any_exc) { // workgroup-uniform
		if (tid < 32 * V) { L[tid >> 5].mask[tid & 31] = 0; }
		asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); // not __syncthreads(): its fence would wait for the loads in flight
#pragma unroll
		for (int i = 0; i < V; ++i) { land_exceptions<VB>(L[i], d[i], excs + d[i].exc_off, pos[i], tid); }
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // LDS-DMA completion is not tracked through the LDS for the compiler
	__syncthreads();
}

// a per-vector result of the sinks: the adjacent-lane tree over the 64 lane totals (DPP, alp_device.hpp), stored by lane 0 as a count (u32) or a double
template <bool AS_COUNT>
__device__ __forceinline__ void store_vector_result(double* __restrict__ out, uint64_t v, double total, int lane) {
	total = wave_tree_sum_f64(total);
	if (lane == 0) {
		if constexpr (AS_COUNT) {
			reinterpret_cast<uint32_t*>(out)[v] = static_cast<uint32_t>(total);
		} else {
			out[v] = total;
		}
	}
}

// Per-vector results of the workgroup sinks: lane partial acc[i] (step order) in each of the four wavefronts -> the four partials of a lane position combined as
// (w0 + w1) + (w2 + w3) -> ONE adjacent-lane tree over the 64 results, by one wavefront per vector.  (Counts take the same route; they
// are small integers, so the order does not matter.)  Until late in round 3 every wavefront ran its own tree first: 18 of the ~125
// vector instructions per wavefront and vector of a kernel whose VALU is 100 % busy (profiles/r03_consumers.txt).  The lane partials
// travel through the vectors' packed-word stages, which every wavefront is done with behind the first barrier here.  before_tree(i, total): what
// the wavefront that finishes vector i adds to its lane totals in front of the tree.  tests/test_decode_sum_gpu.py replays this order on the host.
template <bool AS_COUNT, int V, class LDS, class HOOK>
__device__ __forceinline__ void finish_vector_sinks(LDS (&L)[V], const double (&acc)[V], double* __restrict__ out, uint64_t v0, uint64_t n_vectors, int wave, int lane,
                                                    HOOK before_tree) {
	__syncthreads(); // nobody reads packed words any more
	static_assert(LDS::kStage >= 8 * kDecThreads && kDecWaves == 4 && V <= kDecWaves, "the lane partials of a vector fit its stage; the documented summation order is for 4 wavefronts per vector");
#pragma unroll
	for (int i = 0; i < V; ++i) { reinterpret_cast<double*>(L[i].stage)[64 * wave + lane] = acc[i]; }
	__syncthreads();
	if (wave < V && v0 + wave < n_vectors) { // wave-uniform: wavefront w finishes vector w
		const double* part  = reinterpret_cast<const double*>(L[wave].stage) + lane;
		double        total = (part[0] + part[64]) + (part[128] + part[192]);
#pragma unroll
		for (int i = 0; i < V; ++i) {
			if (wave == i) { before_tree(i, total); }
		}
		store_vector_result<AS_COUNT>(out, v0 + wave, total, lane);
	}
}

// ---- the one-wavefront kernels (k_sink_direct, k_sink_direct_f32): a wavefront owns a vector and its own LDS record, no barrier -----------------------------
// staged (wave-uniform, the caller's rule): the vector's packed words whole into the wavefront's LDS by LDS-DMA (1 KiB per instruction, no registers) — ONE round
// trip for all of them instead of batches of register loads: what took the double sink from 0.85 to 0.73 ms (profiles/r03_consumers.txt).  The caller waits
// (vmcnt(0), wave_lds_sync) before it reads them.  A vector with exceptions: the values of the first LDS::kExcBytes / VB by LDS-DMA, the mask from the
// positions, its prefix into L.pref; returns the mask as this wavefront sees it.
template <int VB, class LDS>
__device__ __forceinline__ ExcMask stage_wave_vector(LDS& L, const alpgpu_vector_desc& d, const uint8_t* __restrict__ packed, const uint8_t* __restrict__ rec, bool staged,
                                                     int lane) {
	const bool is_alp = d.scheme == ALPGPU_SCHEME_ALP;
	const int  cnt    = d.exc_cnt;
	ExcMask    em {0u, 0};
	if (staged) {
		typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
		const ull2* g       = reinterpret_cast<const ull2*>(packed + d.packed_off);
		const int   n_units = 8 * (d.bw + (is_alp ? 0 : d.lbw));
		for (int j = 0; 64 * j < n_units; ++j) {
			if (64 * j + lane < n_units) { __builtin_amdgcn_global_load_lds(g + 64 * j + lane, reinterpret_cast<ull2*>(L.stage) + 64 * j, 16, 0, 0); }
		}
	}
	if (cnt > 0) { // wave-uniform
		const uint32_t val_bytes = (is_alp ? static_cast<uint32_t>(VB) : 2u) * static_cast<uint32_t>(cnt);
		const int      dwords    = static_cast<int>(((val_bytes < LDS::kExcBytes ? val_bytes : LDS::kExcBytes) + 3u) >> 2);
		for (int q = 0; 64 * q < dwords; ++q) { // wave-uniform trip count; LDS destination = wave-uniform base + 4 * lane
			if (64 * q + lane < dwords) { __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint32_t*>(rec) + 64 * q + lane, reinterpret_cast<uint32_t*>(L.excv) + 64 * q, 4, 0, 0); }
		}
		if (lane < 32) { L.mask[lane] = 0u; }
		wave_lds_sync();
		const uint16_t* poss = reinterpret_cast<const uint16_t*>(rec + val_bytes);
		for (int j = lane; j < cnt; j += 64) {
			const uint32_t p = poss[j];
			atomicOr(&L.mask[p >> 5], 1u << (p & 31u));
		}
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the DMA'd values (LDS-DMA completion is not tracked through the LDS for the compiler)
		wave_lds_sync();
		em = load_exception_mask(L, lane);
		if (lane < 32) { L.pref[lane] = static_cast<uint32_t>(em.excl); }
		wave_lds_sync();
	}
	return em;
}

// ---- launch side (launch.hpp: launch_over_column) ---------------------------------------------------------------------------------------------------
constexpr uint64_t* kNoProgress = nullptr; // a launch that reports to no read-ahead
inline uint64_t     wgs_of(const alpgpu_column* col, uint64_t vectors_per_wg) { return (col->n_vectors + vectors_per_wg - 1) / vectors_per_wg; }
inline dim3         dec_block() { return dim3(kDecThreads); }

} // namespace alpgpu
