// distinct_kernels.hip — distinct values (include/alpgpu.h, "distinct values": alpgpu_distinct_*): the sorted distinct values of a compressed column's
// selected values and their counts.  It walks and decodes as k_histogram does (persistent_scan.hpp) and orders by top-k's key (top_k_device.hpp: top_k_okey), taken after a
// zero has been made +0.0: from there on equal values are equal 64-bit integers (a float's key zero-extended) and everything is integer.
//
//   k_distinct_reset       the global table's keys to EMPTY (all-ones: the order key of a NaN pattern, and NaNs are never inserted), its counts, the
//                          state words and the sort's pairs ({EMPTY, 0}: the padding) by a kernel of the library's own, not a memset node
//                          (mask_kernels.hip, k_fill_u64, says why).
//   k_distinct_insert<VB>  k_histogram's shape: persistent workgroups of kDistWaves wavefronts, ONE barrier in front of the loop, the vectors of the
//                          range v = wave id, wave id + waves, ...; every wavefront of a workgroup makes the same number of trips, so that the flush's
//                          barriers are met by all.  A vector is decoded in registers (register_decode.hpp) in batches of kStepBatch steps.  Per step:
//                          the selected NaNs are one popcount; if the kept lanes agree on their key that is ONE insert with the popcount, otherwise one
//                          insert per kept lane.  The selected numbers are counted by popcounts beside the tables (state word 2): right on overflow too.
//   the LDS table          open addressing, lds_slots keys (64-bit for double, 32-bit for float) and 32-bit counts: atomicCAS(EMPTY -> key) on at most
//                          kDistLdsProbes neighbouring slots, then an LDS add.  A value that finds no place goes straight to the global table.
//   the flush              behind a barrier, at the end and every flush_every trips (default kDistFlushEvery: a trip adds at most 8 x 1024 to one 32-bit
//                          count): every occupied LDS slot into the global table with its count, and emptied.
//   the global table       table_slots (default the power of two >= 2 x capacity) 64-bit keys and, in an array of their own, 64-bit counts: a
//                          multiplicative hash, linear probing, atomicCAS(EMPTY -> key), then atomicAdd on the count.  The lane that claims a slot adds
//                          1 to the claimed counter; a result >= capacity raises the overflow flag, and with the flag up new keys are dropped.
//                          EVERY probe loop is bounded by the slots of the table it walks; a lane that finds no place raises overflow and drops its
//                          value.  No lane waits for anything another lane, wavefront or workgroup does.
//   zones                  ONE shortcut: a record with min == max (no NaN bound) on a vector whose descriptor says ALP without exceptions (only there
//                          a NaN is always an exception) is one insert of that value with the popcount of the selected bits; the packed words are not
//                          requested.  Every other vector is decoded.
//   k_distinct_compact     the occupied slots into the pairs {key, count}: ballot, mbcnt, one atomic add per wavefront, at most capacity entries, in
//                          arbitrary order (the keys are distinct, so the sort gives the same bytes whatever the order).
//   the sort               a bitonic network over the P = power of two >= capacity pairs, ascending by key, the padding {EMPTY, 0} last.
//                          k_distinct_sort_tile: every stride below sort_tile, in LDS, one workgroup per tile; k_distinct_sort_stride: one global
//                          compare-exchange launch per larger stride.  The grids and the launch count are fixed on the host from capacity; with S = the
//                          power of two >= the entries there are, stages beyond S exchange nothing (the pairs [0, S) are sorted and everything behind
//                          them is padding), so workgroups and threads that lie beyond S, or run a stage beyond S, leave at once.
//   k_distinct_emit<VB>    the values back from their keys, the counts if wanted, and the caller's four state words.
//
// HBM traffic per vector: k_histogram's.  The low-cardinality column is the case this exists for: almost every step is the wave-agreement insert or an
// LDS hit, and the global table sees a few entries per workgroup and flush.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; launch bounds 512 = 2 wavefronts per SIMD and workgroup):
//   k_distinct_insert<8>   86 VGPRs, 50180 B LDS, 5 waves per SIMD, no scratch; amdgpu_waves_per_eu(4): TWO workgroups per CU.  The LDS admits three,
//                          but held to the 80 registers that takes the kernel spilled (20 B of scratch, 4 VGPRs), and it must not spill.
//   k_distinct_insert<4>   74 VGPRs, 33796 B LDS, 6 waves per SIMD, no scratch; amdgpu_waves_per_eu(6): the three workgroups per CU the grid is sized for
//   k_distinct_sort_tile   14 VGPRs, 65536 B LDS (two workgroups per CU); the other kernels: at most 14 VGPRs, no LDS, no scratch
// Both insert kernels keep about 75 wave-uniform values that do not fit the scalar file in lanes of two VGPRs (counted above).
#include "persistent_scan.hpp"
#include "top_k_device.hpp"

namespace alpgpu {

constexpr int      kDistWaves       = 8; // wavefronts per workgroup: they share the LDS table
constexpr int      kDistThreads     = 64 * kDistWaves;
constexpr int      kDistWgPerCu     = 3;        // float: 33 KiB of LDS and 6 waves per SIMD each
constexpr int      kDistWgPerCuF64  = 2;        // double: 49 KiB of LDS each, and the registers of 5 waves per SIMD
constexpr uint32_t kDistLdsSlots    = 4096;     // of the workgroup's table
constexpr uint32_t kDistLdsSlotsMin = 64;
constexpr uint32_t kDistLdsProbes   = 8;        // slots an LDS insert looks at before it goes to the global table
constexpr uint32_t kDistFlushEvery  = 1u << 18; // trips of a workgroup's loop (8 vectors each, at most 8192 increments of one 32-bit LDS count) between two flushes
constexpr uint32_t kDistSortTile    = 4096;     // pairs sorted in LDS by one workgroup: 64 KiB
constexpr uint32_t kDistSortTileMin = 64;
constexpr int      kDistSortThreads = 512;
constexpr uint64_t kDistEmpty       = ~0ull;
constexpr uint64_t kDistHashMul     = 0x9E3779B97F4A7C15ull; // 2^64 / the golden ratio
// the words of the state in the scratch (8 of them)
constexpr uint32_t kDistClaimed = 0u, kDistNans = 1u, kDistNumbers = 2u, kDistOverflow = 3u, kDistCompacted = 4u, kDistStateWords = 8u;

struct DistTable {
	uint64_t* keys;   // [1 << log2_slots]
	uint64_t* counts; // [1 << log2_slots]
	uint64_t* state;  // [kDistStateWords]
	uint64_t  capacity;
	uint32_t  log2_slots;
};

struct DistArgs {
	uint64_t        v_begin, v_end; // the vectors that hold a value of the range
	uint64_t        first, end;     // the selected index range
	const uint64_t* mask;           // nullable: every value of the range
	const void*     zones;          // nullable: one record {min, max} per vector
	uint64_t*       trace;          // nullable: 6 words, added to
	DistTable       table;
	uint32_t        log2_lds; // slots of the LDS table
	uint32_t        flush_every;
};

__device__ __forceinline__ unsigned long long* dist_ull(uint64_t* p) { return reinterpret_cast<unsigned long long*>(p); }

// the slot a key's probes begin at in a table of 1 << log2_slots slots: the product's top bits
__device__ __forceinline__ uint32_t dist_hash(uint64_t key, uint32_t log2_slots) {
	return log2_slots == 0u ? 0u : static_cast<uint32_t>((key * kDistHashMul) >> (64u - log2_slots));
}

// the value's key: okey of the value with a zero made +0.0 (x is no NaN where the key is used)
template <int VB>
__device__ __forceinline__ uint64_t dist_key(typename DecodeVec<VB>::T x) {
	typedef typename DecodeVec<VB>::T T;
	if constexpr (VB == 8) { // (by the bits: no floating-point mode has a say in what a zero is)
		return top_k_okey<VB>((static_cast<uint64_t>(__double_as_longlong(x)) << 1) == 0ull ? T(0) : x);
	} else {
		return top_k_okey<VB>((__float_as_uint(x) << 1) == 0u ? T(0) : x);
	}
}

// n occurrences of `key` into the global table.  At most `slots` probes, no waiting: a key that finds neither itself nor a free slot raises the
// overflow flag and is dropped (its values are in state word 2 already).
__device__ __forceinline__ void dist_global_insert(const DistTable& t, uint64_t key, uint64_t n) {
	const uint32_t slots = 1u << t.log2_slots, wrap = slots - 1u;
	uint32_t       at    = dist_hash(key, t.log2_slots);
	for (uint32_t p = 0; p < slots; ++p) {
		uint64_t cur = __hip_atomic_load(&t.keys[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (cur == kDistEmpty) {
			if (__hip_atomic_load(&t.state[kDistOverflow], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) { return; } // new keys are dropped
			cur = atomicCAS(dist_ull(&t.keys[at]), kDistEmpty, key);
			if (cur == kDistEmpty) { // claimed
				if (atomicAdd(dist_ull(&t.state[kDistClaimed]), 1ull) >= t.capacity) { atomicOr(dist_ull(&t.state[kDistOverflow]), 1ull); }
				cur = key;
			}
		}
		if (cur == key) {
			atomicAdd(dist_ull(&t.counts[at]), n);
			return;
		}
		if ((p & 255u) == 255u && __hip_atomic_load(&t.state[kDistOverflow], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) { return; } // a long walk in a call that has failed
		at = (at + 1u) & wrap;
	}
	atomicOr(dist_ull(&t.state[kDistOverflow]), 1ull);
}

// n occurrences of `key` into the workgroup's LDS table; false: no place within kDistLdsProbes slots
template <class KT>
__device__ __forceinline__ bool dist_lds_insert(KT* s_keys, uint32_t* s_counts, uint32_t log2_lds, uint64_t key, uint32_t n) {
	const uint32_t wrap = (1u << log2_lds) - 1u;
	const KT       k    = static_cast<KT>(key), empty = static_cast<KT>(kDistEmpty);
	uint32_t       at   = dist_hash(key, log2_lds);
	for (uint32_t p = 0; p < kDistLdsProbes; ++p) {
		const KT cur = atomicCAS(&s_keys[at], empty, k);
		if (cur == empty || cur == k) {
			atomicAdd(&s_counts[at], n);
			return true;
		}
		at = (at + 1u) & wrap;
	}
	return false;
}

// what a lane counts for the trace
struct DistDid {
	uint32_t agreed;  // steps settled by wave agreement (wave-uniform)
	uint32_t offered; // inserts offered to the LDS table (wave-uniform)
};

// One step's kept lanes (keep: wave-uniform, no NaN among them) with their keys into the LDS table: one insert by the leading lane when they agree.
template <class KT>
__device__ __forceinline__ void dist_offer(KT* s_keys, uint32_t* s_counts, uint32_t* s_made, const DistArgs& g, uint64_t keep, uint64_t key, uint32_t lane, DistDid& did) {
	if (keep == 0ull) { return; } // (wave-uniform)
	const uint32_t lead  = static_cast<uint32_t>(__builtin_ctzll(keep));
	const uint64_t first = readlane64(key, lead);
	const uint32_t kept  = static_cast<uint32_t>(__builtin_popcountll(keep));
	const bool     agree = (ballot64(key != first) & keep) == 0ull;
	const bool     go    = agree ? lane == lead : ((keep >> lane) & 1ull) != 0ull;
	const uint32_t n     = agree ? kept : 1u;
	did.agreed += agree ? 1u : 0u;
	did.offered += agree ? 1u : kept;
	if (go && !dist_lds_insert(s_keys, s_counts, g.log2_lds, key, n)) {
		dist_global_insert(g.table, key, n);
		atomicAdd(s_made, 1u);
	}
}

// every occupied slot of the LDS table into the global table, and emptied; a barrier on both sides
template <class KT>
__device__ __forceinline__ void dist_flush(KT* s_keys, uint32_t* s_counts, uint32_t* s_made, const DistArgs& g) {
	__syncthreads();
	const uint32_t slots = 1u << g.log2_lds;
	for (uint32_t i = threadIdx.x; i < slots; i += kDistThreads) {
		const KT k = s_keys[i];
		if (k != static_cast<KT>(kDistEmpty)) {
			dist_global_insert(g.table, static_cast<uint64_t>(k), static_cast<uint64_t>(s_counts[i]));
			atomicAdd(s_made, 1u);
			s_keys[i]   = static_cast<KT>(kDistEmpty);
			s_counts[i] = 0u;
		}
	}
	__syncthreads();
}

constexpr uint32_t kDistSkipZero = 0u, kDistZone = 1u, kDistDecoded = 2u; // what dist_vector did with a vector: the trace's first words

// One vector by one wavefront.  n_nan, n_num (wave-uniform): the selected NaNs and numbers, moved on.  Returns the class of the trace.
template <int VB, class KT>
__device__ __forceinline__ uint32_t dist_vector(const ColumnStreams& c, const DistArgs& g, uint64_t v, uint32_t wave, uint32_t lane, KT* s_keys, uint32_t* s_counts, uint32_t* s_made,
                                                uint64_t (&s_exc)[kDistWaves][16], uint64_t& n_nan, uint64_t& n_num, DistDid& did) {
	typedef typename DecodeVec<VB>::T T;
	// 1. the selected bits: the vector's 128 bytes of bitmap (all ones without one), lane m < 16 holding word m, ANDed with the range's share
	uint64_t sel; // (the vector holds a value of the range: the loop walks the range's vectors only)
	if (!selected_words(g.mask, g.first, g.end, v, lane, sel)) { return kDistSkipZero; }

	// 2. the one shortcut: a constant vector by its record
	if (g.zones != nullptr) {
		const T* zone = static_cast<const T*>(g.zones) + 2 * v; // (wave-uniform)
		const T  mn = zone[0], mx = zone[1];
		if (mn == mx) { // (false with a NaN bound)
			if (alp_without_exceptions(c.descs[v])) { // no NaN can hide here: the selected bits are the count of the one value
				const uint32_t n = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(selected_count(sel)), 63));
				n_num += n;
				++did.offered;
				if (lane == 0u && !dist_lds_insert(s_keys, s_counts, g.log2_lds, dist_key<VB>(mn), n)) {
					dist_global_insert(g.table, dist_key<VB>(mn), n);
					atomicAdd(s_made, 1u);
				}
				return kDistZone;
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
		// 5. the batch's keys first (the loaded words are dead behind them), the selected NaNs of a step one popcount
		uint64_t key[kStepBatch], keep[kStepBatch];
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			const T        x    = step_value(V, R, b, i, lane);
			const uint64_t w    = readlane64(sel, b + i);
			const uint64_t nans = ballot64(top_k_is_nan<VB>(x));
			key[i]              = dist_key<VB>(x);
			keep[i]             = w & ~nans;
			n_nan += static_cast<uint32_t>(__builtin_popcountll(w & nans));
			n_num += static_cast<uint32_t>(__builtin_popcountll(keep[i]));
		}
		// 6. per step: the selected numbers go to the table by their keys
		// (a loop that stays a loop, its operands selected: one copy of the insert's code and of its registers)
		static_assert(kStepBatch == 4u, "the selects below");
#pragma nounroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			const uint64_t k = i == 0u ? key[0] : i == 1u ? key[1] : i == 2u ? key[2] : key[3];
			const uint64_t w = i == 0u ? keep[0] : i == 1u ? keep[1] : i == 2u ? keep[2] : keep[3];
			dist_offer(s_keys, s_counts, s_made, g, w, k, lane, did);
		}
	}
	return kDistDecoded;
}

// (float: 6 wavefronts per SIMD are 3 workgroups per CU, what the LDS admits; double: 4, see the head of the file)
template <int VB>
__global__ __launch_bounds__(kDistThreads) __attribute__((amdgpu_waves_per_eu(VB == 8 ? 4 : 6))) void k_distinct_insert(const ColumnStreams c, const DistArgs g) {
	typedef typename std::conditional<VB == 8, unsigned long long, uint32_t>::type KT;
	__shared__ KT       s_keys[kDistLdsSlots];
	__shared__ uint32_t s_counts[kDistLdsSlots];
	__shared__ uint64_t s_exc[kDistWaves][16]; // per wavefront: bit p = value p is an exception
	__shared__ uint32_t s_made;                // inserts the workgroup made into the global table (the trace's word 5)

	const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const uint32_t lane = threadIdx.x & 63u;

	// 0. the table emptied, once per workgroup; the one barrier in front of the loop
	for (uint32_t i = threadIdx.x; i < (1u << g.log2_lds); i += kDistThreads) {
		s_keys[i]   = static_cast<KT>(kDistEmpty);
		s_counts[i] = 0u;
	}
	if (threadIdx.x == 0u) { s_made = 0u; }
	__syncthreads();

	// every wavefront of the workgroup makes the same number of trips (the last may find no vector), so that the flush's barriers are met by all
	const uint64_t n_waves = static_cast<uint64_t>(gridDim.x) * kDistWaves;
	uint64_t       n_nan = 0, n_num = 0;
	DistDid        did {0u, 0u};
	uint32_t       what_did[3] = {0u, 0u, 0u};
	uint32_t       trips       = 0;
	for (uint64_t k0 = g.v_begin + static_cast<uint64_t>(blockIdx.x) * kDistWaves; k0 < g.v_end; k0 += n_waves) {
		const uint64_t v = k0 + wave;
		if (v < g.v_end) {
			const uint32_t what = dist_vector<VB, KT>(c, g, v, wave, lane, s_keys, s_counts, &s_made, s_exc, n_nan, n_num, did);
#pragma unroll
			for (uint32_t i = 0; i < 3u; ++i) { what_did[i] += what == i ? 1u : 0u; }
		}
		if (++trips == g.flush_every) {
			trips = 0;
			dist_flush(s_keys, s_counts, &s_made, g);
		}
	}
	dist_flush(s_keys, s_counts, &s_made, g);
	// the wavefront's selected NaNs and numbers: one add each
	if (lane == 0u) {
		if (n_nan != 0ull) { atomicAdd(dist_ull(&g.table.state[kDistNans]), n_nan); }
		if (n_num != 0ull) { atomicAdd(dist_ull(&g.table.state[kDistNumbers]), n_num); }
	}
	if (g.trace != nullptr) {
		if (lane < 5u) { // one add per wavefront and counter
			const uint32_t mine = lane == 0u ? what_did[0] : lane == 1u ? what_did[1] : lane == 2u ? what_did[2] : lane == 3u ? did.agreed : did.offered;
			if (mine != 0u) { atomicAdd(dist_ull(g.trace) + lane, static_cast<unsigned long long>(mine)); }
		}
		if (threadIdx.x == 0u && s_made != 0u) { atomicAdd(dist_ull(g.trace) + 5, static_cast<unsigned long long>(s_made)); } // (behind the last flush's barrier)
	}
}

// The call's "memset" (k_fill_u64, mask_kernels.hip, says why it is a kernel): table_slots keys to EMPTY and counts to 0, sort_slots pairs to the padding, the state
__global__ __launch_bounds__(256) void k_distinct_reset(uint64_t* __restrict__ keys, uint64_t* __restrict__ counts, ulonglong2* __restrict__ pairs, uint64_t* __restrict__ state,
                                                        uint32_t table_slots, uint32_t sort_slots) {
	uint32_t most = table_slots > sort_slots ? table_slots : sort_slots;
	most          = most > kDistStateWords ? most : kDistStateWords; // (a table of one or two slots is shorter than the state)
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < most; i += gridDim.x * 256u) {
		if (i < table_slots) {
			keys[i]   = kDistEmpty;
			counts[i] = 0ull;
		}
		if (i < sort_slots) { pairs[i] = make_ulonglong2(kDistEmpty, 0ull); }
		if (i < kDistStateWords) { state[i] = 0ull; }
	}
}

// The occupied slots into pairs[0 .. capacity): a wavefront looks at 64 neighbouring slots, one atomic add for those it found occupied.
__global__ __launch_bounds__(256) void k_distinct_compact(const DistTable t, ulonglong2* __restrict__ pairs) {
	const uint32_t slots = 1u << t.log2_slots;
	const uint32_t lane  = threadIdx.x & 63u;
	for (uint32_t base = blockIdx.x * 256u + (threadIdx.x & ~63u); base < slots; base += gridDim.x * 256u) { // (wave-uniform)
		const uint32_t i        = base + lane;
		const uint64_t key      = i < slots ? t.keys[i] : kDistEmpty;
		const uint64_t occupied = ballot64(key != kDistEmpty);
		if (occupied == 0ull) { continue; }
		uint64_t at = 0;
		if (lane == 0u) { at = atomicAdd(dist_ull(&t.state[kDistCompacted]), static_cast<unsigned long long>(__builtin_popcountll(occupied))); }
		at = readlane64(at, 0u) + mbcnt64(occupied, 0u);
		if (key != kDistEmpty && at < t.capacity) { pairs[at] = make_ulonglong2(key, t.counts[i]); }
	}
}

// S: the power of two at or above the entries the compaction wrote (at least 1).  The pairs [S, P) are padding.
__device__ __forceinline__ uint32_t dist_sort_span(const uint64_t* state, uint64_t capacity) {
	const uint64_t found = state[kDistCompacted];
	const uint32_t n     = static_cast<uint32_t>(found < capacity ? found : capacity);
	return n <= 1u ? 1u : 1u << (32u - static_cast<uint32_t>(__builtin_clz(n - 1u)));
}

// The bitonic stages k = k_lo, 2 k_lo, ..., k_hi of the pairs [tile * blockIdx.x, + tile), every stride below `tile` (a power of two in 2 ..
// kDistSortTile, k_lo >= 2): the first launch runs k = 2 .. tile whole, the later ones the tail of one stage k > tile.  Ascending where bit k of the
// pair's index is clear.
__global__ __launch_bounds__(kDistSortThreads) void k_distinct_sort_tile(ulonglong2* __restrict__ pairs, const uint64_t* __restrict__ state, uint64_t capacity, uint32_t tile,
                                                                         uint32_t k_lo, uint32_t k_hi) {
	__shared__ uint64_t s_key[kDistSortTile];
	__shared__ uint64_t s_cnt[kDistSortTile];
	const uint32_t span = dist_sort_span(state, capacity);
	const uint32_t base = blockIdx.x * tile;
	if (base >= span || k_lo > span) { return; } // (the workgroup as one) nothing but padding, or a stage that exchanges nothing
	if (k_hi > span) { k_hi = span; }
	for (uint32_t i = threadIdx.x; i < tile; i += kDistSortThreads) {
		const ulonglong2 p = pairs[base + i];
		s_key[i]           = p.x;
		s_cnt[i]           = p.y;
	}
	for (uint32_t k = k_lo; k <= k_hi; k <<= 1) {
		for (uint32_t j = (k >> 1) < (tile >> 1) ? (k >> 1) : (tile >> 1); j > 0u; j >>= 1) {
			__syncthreads();
			for (uint32_t t = threadIdx.x; t < (tile >> 1); t += kDistSortThreads) {
				const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), p = i | j; // (i < p < tile)
				const bool     ascending = ((base + i) & k) == 0u;
				const uint64_t a = s_key[i], b = s_key[p];
				if (ascending ? a > b : a < b) {
					const uint64_t ca = s_cnt[i], cb = s_cnt[p];
					s_key[i] = b, s_key[p] = a;
					s_cnt[i] = cb, s_cnt[p] = ca;
				}
			}
		}
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < tile; i += kDistSortThreads) { pairs[base + i] = make_ulonglong2(s_key[i], s_cnt[i]); }
}

// One compare-exchange of stage k at stride j >= the tile, over the n_pairs / 2 comparators
__global__ __launch_bounds__(256) void k_distinct_sort_stride(ulonglong2* __restrict__ pairs, const uint64_t* __restrict__ state, uint64_t capacity, uint32_t n_half, uint32_t k,
                                                              uint32_t j) {
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	if (t >= n_half) { return; }
	const uint32_t span = dist_sort_span(state, capacity);
	const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), p = i | j; // (i < p < 2 n_half)
	if (k > span || i >= span) { return; }                                // the stage exchanges nothing there
	const bool       ascending = (i & k) == 0u;
	const ulonglong2 a = pairs[i], b = pairs[p];
	if (ascending ? a.x > b.x : a.x < b.x) {
		pairs[i] = b;
		pairs[p] = a;
	}
}

template <int VB>
__global__ __launch_bounds__(256) void k_distinct_emit(const ulonglong2* __restrict__ pairs, const uint64_t* __restrict__ state, uint64_t capacity,
                                                       typename DecodeVec<VB>::U* __restrict__ vals, uint64_t* __restrict__ counts, uint64_t* __restrict__ d_state) {
	typedef typename DecodeVec<VB>::U U;
	const uint64_t claimed = state[kDistClaimed];
	const uint64_t n       = claimed < capacity ? claimed : capacity;
	const uint64_t i       = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
	if (i < n) {
		const ulonglong2 p = pairs[i];
		vals[i]            = static_cast<U>(top_k_bits_of_hi<VB>(p.x, true));
		if (counts != nullptr) { counts[i] = p.y; }
	}
	if (i == 0u) {
		d_state[0] = n;
		d_state[1] = state[kDistNans];
		d_state[2] = state[kDistNumbers];
		d_state[3] = state[kDistOverflow] != 0ull || claimed > capacity ? 1ull : 0ull;
	}
}

static uint32_t pow2_at_or_below(uint32_t x) { // x >= 1
	uint32_t p = 1;
	while (2ull * p <= x) { p <<= 1; }
	return p;
}
static uint32_t log2_of(uint64_t pow2) {
	uint32_t l = 0;
	while ((1ull << l) < pow2) { ++l; }
	return l;
}

// col->n_vectors > 0, n > 0, capacity in 1 .. ALPGPU_DISTINCT_MAX; range and alignments checked by the caller
int launch_distinct(hipStream_t stream, const alpgpu_column* col, uint64_t first, uint64_t n, const uint64_t* d_mask, const void* d_zones, uint64_t capacity, void* d_vals,
                    uint64_t* d_counts, uint64_t* d_state, void* d_scratch, int value_bytes, int n_cus, const alpgpu_distinct_tuning* tuning, uint64_t* d_trace) {
	DistinctLayout L;
	if (!distinct_layout(capacity, L)) { return ALPGPU_ERR_INVALID; }
	uint8_t*    scratch = static_cast<uint8_t*>(d_scratch);
	ulonglong2* pairs   = reinterpret_cast<ulonglong2*>(scratch + L.pairs);
	// what the tuning record may lower
	uint32_t table_slots = static_cast<uint32_t>(L.table_slots), lds_slots = kDistLdsSlots, sort_tile = kDistSortTile, flush_every = kDistFlushEvery;
	if (tuning != nullptr) {
		if (tuning->table_slots != 0u && tuning->table_slots < table_slots) {
			const uint32_t t = pow2_at_or_below(tuning->table_slots);
			table_slots      = t < L.sort_slots ? static_cast<uint32_t>(L.sort_slots) : t;
		}
		if (tuning->lds_slots != 0u && tuning->lds_slots < lds_slots) { lds_slots = tuning->lds_slots < kDistLdsSlotsMin ? kDistLdsSlotsMin : pow2_at_or_below(tuning->lds_slots); }
		if (tuning->sort_tile != 0u && tuning->sort_tile < sort_tile) { sort_tile = tuning->sort_tile < kDistSortTileMin ? kDistSortTileMin : pow2_at_or_below(tuning->sort_tile); }
		if (tuning->flush_every != 0u && tuning->flush_every < flush_every) { flush_every = tuning->flush_every; }
	}
	DistArgs args {};
	args.v_begin          = first >> 10;
	args.v_end            = (first + n + 1023u) >> 10;
	args.first            = first;
	args.end              = first + n;
	args.mask             = d_mask;
	args.zones            = d_zones;
	args.trace            = d_trace;
	args.table.keys       = reinterpret_cast<uint64_t*>(scratch + L.keys);
	args.table.counts     = reinterpret_cast<uint64_t*>(scratch + L.counts);
	args.table.state      = reinterpret_cast<uint64_t*>(scratch + L.state);
	args.table.capacity   = capacity;
	args.table.log2_slots = log2_of(table_slots);
	args.log2_lds         = log2_of(lds_slots);
	args.flush_every      = flush_every;

	// 1. the reset
	const uint32_t sort_slots = static_cast<uint32_t>(L.sort_slots);
	const uint32_t most       = table_slots > sort_slots ? table_slots : sort_slots;
	const unsigned reset_grid = (most + 255u) / 256u < 2048u ? (most + 255u) / 256u : 2048u;
	hipLaunchKernelGGL(k_distinct_reset, dim3(reset_grid), dim3(256), 0, stream, args.table.keys, args.table.counts, pairs, args.table.state, table_slots, sort_slots);
	if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }

	// 2. the inserts: the grid is sized to the device
	const unsigned grid = persistent_grid(args.v_end - args.v_begin, kDistWaves, n_cus, value_bytes == 8 ? kDistWgPerCuF64 : kDistWgPerCu, 0,
	                                      tuning != nullptr ? tuning->grid : 0u, kTuningGridMax);
	const ColumnStreams c = column_streams(col);
	if (value_bytes == 8) {
		hipLaunchKernelGGL((k_distinct_insert<8>), dim3(grid), dim3(kDistThreads), 0, stream, c, args);
	} else {
		hipLaunchKernelGGL((k_distinct_insert<4>), dim3(grid), dim3(kDistThreads), 0, stream, c, args);
	}
	if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }

	// 3. the compaction
	const unsigned compact_grid = (table_slots + 255u) / 256u < 2048u ? (table_slots + 255u) / 256u : 2048u;
	hipLaunchKernelGGL(k_distinct_compact, dim3(compact_grid), dim3(256), 0, stream, args.table, pairs);
	if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }

	// 4. the sort: the strides below the tile in LDS, one launch per larger stride
	if (sort_slots >= 2u) {
		const uint32_t tile   = sort_tile < sort_slots ? sort_tile : sort_slots;
		const unsigned n_tile = sort_slots / tile;
		const uint32_t n_half = sort_slots / 2u;
		hipLaunchKernelGGL(k_distinct_sort_tile, dim3(n_tile), dim3(kDistSortThreads), 0, stream, pairs, args.table.state, capacity, tile, 2u, tile);
		for (uint32_t k = 2u * tile; k != 0u && k <= sort_slots; k <<= 1) {
			for (uint32_t j = k >> 1; j >= tile; j >>= 1) {
				hipLaunchKernelGGL(k_distinct_sort_stride, dim3((n_half + 255u) / 256u), dim3(256), 0, stream, pairs, args.table.state, capacity, n_half, k, j);
			}
			hipLaunchKernelGGL(k_distinct_sort_tile, dim3(n_tile), dim3(kDistSortThreads), 0, stream, pairs, args.table.state, capacity, tile, k, k);
		}
		if (hipGetLastError() != hipSuccess) { return ALPGPU_ERR_HIP; }
	}

	// 5. the emit
	const unsigned emit_grid = static_cast<unsigned>((capacity + 255u) / 256u);
	if (value_bytes == 8) {
		hipLaunchKernelGGL((k_distinct_emit<8>), dim3(emit_grid), dim3(256), 0, stream, pairs, args.table.state, capacity, static_cast<uint64_t*>(d_vals), d_counts, d_state);
	} else {
		hipLaunchKernelGGL((k_distinct_emit<4>), dim3(emit_grid), dim3(256), 0, stream, pairs, args.table.state, capacity, static_cast<uint32_t*>(d_vals), d_counts, d_state);
	}
	return hipGetLastError() != hipSuccess ? ALPGPU_ERR_HIP : ALPGPU_OK;
}

} // namespace alpgpu
