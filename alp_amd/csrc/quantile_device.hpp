// quantile_device.hpp — quantiles (include/alpgpu.h, "quantiles": alpgpu_select_rank_*, alpgpu_quantile_*): the state of the radix select in device
// memory, the slot search and the per-vector step of k_quantile_wide, on the in-register decode of register_decode.hpp and the order of
// top_k_device.hpp (top_k_okey, top_k_is_nan, top_k_bits_of_hi).  Everything that is counted is an integer and every key is exact, so the result
// is a function of the inputs alone.
//
// The select: 8-bit digits of okey(x), most significant first, VB passes.  A RANK is one order statistic looked for (at most kQSlots = 32 of them:
// the caller's ranks, or two per quantile); after pass d it has a settled PREFIX (the top d + 1 bytes of its key, the rest zero), the rank REMaining
// among the values that carry the prefix, and their CouNT.  Ranks that share a prefix share a SLOT: the distinct prefixes, ascending, and one
// histogram of 256 bins per slot and pass.  The ranks themselves need no order: the pick rebuilds the slots from whatever prefixes it finds
// ("Quantiles", says why the host does not sort them).
#pragma once
#include "persistent_scan.hpp"
#include "top_k_device.hpp"

namespace alpgpu {

constexpr uint32_t kQSlots    = ALPGPU_RANK_MAX;
constexpr int      kQWaves    = 8; // wavefronts per workgroup of k_quantile_wide / _narrow: they share the bins and the slot prefixes
constexpr int      kQThreads  = 64 * kQWaves;
constexpr int      kQWgPerCu  = 3;       // 50 KiB of LDS each
constexpr uint32_t kQFlushEvery = 1u << 18; // trips of a workgroup's loop (8 vectors each, at most 8192 increments of one 32-bit LDS bin) between two flushes
constexpr uint32_t kQDecoded = 0u, kQSkipZero = 1u, kQSkipZone = 2u; // what q_vector did with a vector (the trace counts the skips)
constexpr uint32_t kQPlain = 0u, kQCompact = 1u, kQNarrow = 2u; // what pass d does: a wide pass, a wide pass that also appends the candidates, a pass over the candidates

struct QRank {
	uint64_t prefix; // the digits settled so far, the rest zero; after the last pass: the key
	uint64_t rem;    // the value looked for is the rem-th (0-based, ascending) of those that match the prefix
	uint64_t cnt;    // how many match the prefix
	uint32_t slot;   // its histogram in the next pass
	uint32_t pad;
};

// Zeroed by the call's memset together with the bins.
struct QState {
	uint64_t n;          // N: selected values that are no NaNs (pick of pass 0)
	uint64_t n_cand;     // candidates appended (may pass the capacity: readers clamp)
	uint64_t set_bits;   // of the bitmap (k_quantile_popcount)
	uint32_t n_slots;    // distinct prefixes, for the next pass
	uint32_t mode;       // kQPlain / kQCompact / kQNarrow of the next pass (pass 0: from set_bits, q_mode)
	uint32_t compact_p1; // trace: 1 + the pass that appended the candidates, 0: none did
	uint32_t wide_grid, waves_per_wg; // trace (k_quantile_finish)
	uint32_t vb;                      // trace: the passes of the call, 8 or 4
	uint64_t zero_skips;    // trace: vectors whose 16 bitmap words were zero (pass 0)
	uint64_t zone_skips[8]; // trace: vectors skipped by their record, per pass
	uint64_t slot_prefix[kQSlots];
	uint64_t resolved[kQSlots]; // the rank of each entry once N is known
	QRank    rank[kQSlots];
};

// what the caller asked for, as kernel arguments: n ranks (from_top: counted from the largest) or n / 2 quantiles, two ranks each
struct QRequest {
	uint64_t ranks[kQSlots];
	double   q[kQSlots / 2];
	uint32_t n;        // entries: ranks, or 2 * quantiles
	uint32_t quantile; // 0: ranks, 1: q
	uint32_t from_top;
	uint32_t pad;
};

__device__ __forceinline__ uint32_t q_mode(const QState* st, uint32_t pass, uint64_t capacity) {
	return pass == 0u ? (st->set_bits <= capacity ? kQCompact : kQPlain) : st->mode;
}

// the slot whose prefix equals pfx among the n_slots (1 .. kQSlots, wave-uniform) ascending prefixes in LDS: a branch-free lower bound, every lane
// the same steps, then one equality test.  false: pfx is no slot's prefix
__device__ __forceinline__ bool q_find_slot(const uint64_t* s_pfx, uint32_t n_slots, uint64_t pfx, uint32_t& slot) {
	uint32_t base = 0u, n = n_slots;
	while (n > 1u) {
		const uint32_t half = n >> 1;
		base += s_pfx[base + half - 1u] < pfx ? half : 0u;
		n -= half;
	}
	base += s_pfx[base] < pfx ? 1u : 0u; // (base < n_slots here)
	slot = base < kQSlots - 1u ? base : kQSlots - 1u;
	return base < n_slots && s_pfx[slot] == pfx;
}

// One add per kept lane into bins[idx] of the workgroup's LDS histogram; when every kept lane has the same idx (real columns have one or two distinct
// top bytes, a constant column one in every pass) the wavefront adds the popcount once, instead of 64 lanes serialising on one word.
__device__ __forceinline__ void q_hist_add(uint32_t* s_bins, uint64_t keep, uint32_t idx, uint32_t lane) {
	if (keep == 0ull) { return; } // (wave-uniform)
	const uint32_t lead  = static_cast<uint32_t>(__builtin_ctzll(keep));
	const uint32_t first = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(idx), static_cast<int>(lead)));
	const bool     mine  = (keep >> lane) & 1ull;
	if ((ballot64(idx != first) & keep) == 0ull) {
		if (lane == lead) { atomicAdd(&s_bins[first], static_cast<uint32_t>(__builtin_popcountll(keep))); }
	} else if (mine) {
		atomicAdd(&s_bins[idx], 1u);
	}
}

struct QWideArgs {
	uint64_t        n_vectors;
	const uint64_t* mask;     // only read
	const void*     zones;    // nullable: records that contain the vectors' masked intervals
	QState*         st;
	uint64_t*       bins;     // of this pass: [kQSlots][256]
	uint64_t*       cand;     // [capacity] keys
	uint64_t        capacity;
	uint64_t        mask_hi;  // the key's bits above this pass's digit
	uint32_t        shift;    // the digit is bits [shift, shift + 8) of the key
	uint32_t        pass;
	uint32_t        flush_every;
};

// The candidates of a compacting pass are staged per wavefront in kQStageKeys keys of LDS and appended kQStageKeys - 64 or more at a time: one atomic
// add on the one candidate counter per append.  (An add per batch of four steps, the code of k_top_k_candidates, is an add per 256 values of the column
// here: measured, 4 Mi adds on one word took 47 ms of a pass that decodes in 2: profiles/r20_quantile.txt.)  Every place is clamped against the
// capacity, so records that lie cannot make the kernel write outside the array.
constexpr uint32_t kQStageKeys = 256;
__device__ __forceinline__ void q_append(const QWideArgs& g, const uint64_t* s_keys, uint32_t fill, uint32_t lane) {
	if (fill == 0u) { return; } // (wave-uniform)
	uint64_t base = 0;
	if (lane == 0u) { base = atomicAdd(reinterpret_cast<unsigned long long*>(&g.st->n_cand), static_cast<unsigned long long>(fill)); }
	base = readlane64(base, 0u);
	wave_lds_sync();
	for (uint32_t i = lane; i < fill; i += 64u) {
		if (base + i < g.capacity) { g.cand[base + i] = s_keys[i]; }
	}
	wave_lds_sync(); // the keys are read before the next are staged
}

// One vector by one wavefront: its 128 bytes of bitmap, with zones its record against the slots' intervals, then the decode in registers, kStepBatch
// steps at a time.  Every selected value that is no NaN and whose prefix is a slot's is counted in that slot's bin of its digit and, in a compacting
// pass, staged for the candidates at s_keys[fill ...] (the wavefront's own keys; the place of a lane from mbcnt; fill <= kQStageKeys - 64 on entry and
// on return).  Returns kQDecoded or the skip it took.
template <int VB, bool COMPACT, int WAVES>
__device__ __forceinline__ uint32_t q_vector(const ColumnStreams& c, const QWideArgs& g, uint64_t v, uint32_t wave, uint32_t lane, uint32_t n_slots, uint32_t* s_bins,
                                             const uint64_t* s_pfx, uint64_t (&s_exc)[WAVES][16], uint64_t* s_keys, uint32_t& fill) {
	typedef typename DecodeVec<VB>::T T;
	uint64_t prior;
	if (!bitmap_words(g.mask, v, lane, prior)) { return kQSkipZero; }
	if (g.zones != nullptr && g.pass > 0u) {
		const T* zone = static_cast<const T*>(g.zones) + 2 * v; // (wave-uniform)
		const T  mn = zone[0], mx = zone[1];
		if (!top_k_is_nan<VB>(mn) && !top_k_is_nan<VB>(mx)) { // a record with a NaN bound prunes nothing
			const uint64_t kmin = top_k_okey<VB>(mn), kmax = top_k_okey<VB>(mx);
			const uint64_t low  = ~g.mask_hi & (VB == 8 ? ~0ull : 0xFFFFFFFFull);
			const uint64_t p    = s_pfx[lane & (kQSlots - 1u)];
			// slot s holds the keys [p, p | low]: the record meets it or no value of the vector counts there
			if (ballot64(lane < n_slots && kmin <= (p | low) && kmax >= p) == 0ull) { return kQSkipZone; }
		}
	}
	const DecodeVec<VB> A = decode_vec_load<VB>(c, v);
	exception_mask(A, s_exc, wave, lane);

	uint32_t exc_a = 0; // exceptions of the steps done
	for (uint32_t b = 0; b < 16u; b += kStepBatch) {
		StepBatch<VB, kStepBatch> Ra;
		step_request(A, s_exc[wave], b, lane, exc_a, Ra);
#pragma unroll
		for (uint32_t i = 0; i < kStepBatch; ++i) {
			const T        x   = step_value(A, Ra, b, i, lane);
			const uint64_t w   = readlane64(prior, b + i);
			const uint64_t key = top_k_okey<VB>(x);
			uint32_t       slot;
			const bool     match = q_find_slot(s_pfx, n_slots, key & g.mask_hi, slot);
			const uint64_t keep  = w & ballot64(!top_k_is_nan<VB>(x)) & ballot64(match);
			q_hist_add(s_bins, keep, 256u * slot + static_cast<uint32_t>((key >> g.shift) & 255ull), lane);
			if (COMPACT && keep != 0ull) { // (wave-uniform)
				if ((keep >> lane) & 1ull) { s_keys[fill + mbcnt64(keep, 0u)] = key; }
				fill += static_cast<uint32_t>(__builtin_popcountll(keep));
				if (fill > kQStageKeys - 64u) {
					q_append(g, s_keys, fill, lane);
					fill = 0u;
				}
			}
		}
	}
	return kQDecoded;
}

} // namespace alpgpu
