// mask_test.cpp — alp::gpu::column<PT>::select_mask / mask_indices / sum_masked (include/alp/batch.hpp; include/alpgpu.h, "selection bitmaps")
// against a host scan of alp::gpu::column<PT>::decompress of the same blobs: one predicate, two predicates on two columns combined with AND and
// with OR, the indices of the set bits, and SUM / COUNT of a third column under the mask — the sum bit for bit, by a host replica of the order
// the header documents (lane L adds values 64 m + L, m ascending; adjacent-lane tree; the column's total by alpgpu_tree_sum_f64's tree).  Double
// and float columns with ALP and ALP_RD rowgroups, exceptions, specials and an incomplete last vector whose padding must never be selected.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/mask_test.cpp -Lalp_amd -lalpgpu -ldl && ./a.out
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <stdexcept>
#include <vector>

#include "alp.hpp"
#include "alp/batch.hpp"

static int failures = 0;
#define EXPECT(cond, ...)                                                                                              \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			++failures;                                                                                                \
			std::printf("FAIL %s:%d: ", __FILE__, __LINE__);                                                           \
			std::printf(__VA_ARGS__);                                                                                  \
			std::printf("\n");                                                                                         \
		}                                                                                                              \
	} while (0)

template <class PT>
std::vector<PT> make_column(size_t n_values, unsigned seed) {
	std::mt19937_64                        rng(seed);
	std::uniform_real_distribution<double> uni(-1e4, 1e4), unit(0.0, 1.0);
	std::vector<PT>                        v(n_values);
	for (size_t i = 0; i < n_values; ++i) {
		const size_t rg = i / (100 * 1024);
		if (rg % 2 == 1) {
			v[i] = static_cast<PT>(unit(rng)); // full precision: ALP_RD rowgroups
		} else {
			v[i] = static_cast<PT>(std::round(uni(rng) * 100.0) / 100.0);
			if ((rng() & 127) == 0) { v[i] = static_cast<PT>(uni(rng) * 3.14159265358979); }
			if ((rng() & 1023) == 0) { v[i] = (rng() & 1) ? -0.0 : std::numeric_limits<PT>::quiet_NaN(); }
		}
	}
	return v;
}

// s[i] = s[2i] + s[2i + 1], level by level, over a power-of-two count
static double pair_tree(std::vector<double> s) {
	for (size_t w = s.size() / 2; w >= 1; w /= 2) {
		for (size_t i = 0; i < w; ++i) { s[i] = s[2 * i] + s[2 * i + 1]; }
	}
	return s[0];
}

// the documented order of alpgpu_decode_sum_masked_* followed by alpgpu_tree_sum_f64
template <class PT>
static double host_sum_masked(const std::vector<PT>& all, const std::vector<bool>& bit, size_t n_vectors) {
	std::vector<double> sums(n_vectors);
	for (size_t v = 0; v < n_vectors; ++v) {
		std::vector<double> lane(64, 0.0);
		for (size_t m = 0; m < 16; ++m) {
			for (size_t l = 0; l < 64; ++l) {
				const size_t r = 1024 * v + 64 * m + l;
				if (r < bit.size() && bit[r]) { lane[l] += static_cast<double>(all[r]); }
			}
		}
		sums[v] = pair_tree(lane);
	}
	while (true) {
		const size_t        blocks = (sums.size() + 1023) / 1024;
		std::vector<double> next(blocks);
		for (size_t b = 0; b < blocks; ++b) {
			std::vector<double> e(1024, 0.0);
			for (size_t i = 0; i < 1024 && 1024 * b + i < sums.size(); ++i) { e[i] = sums[1024 * b + i]; }
			next[b] = pair_tree(e);
		}
		if (blocks == 1) { return next[0]; }
		sums = next;
	}
}

static void check_mask(const char* name, const char* what, const std::vector<uint64_t>& mask, const std::vector<bool>& want, size_t n_vectors, bool want_some) {
	EXPECT(mask.size() == 16 * n_vectors, "%s %s: %zu mask words, expected %zu", name, what, mask.size(), 16 * n_vectors);
	size_t bad = 0, set = 0;
	for (size_t r = 0; r < 1024 * n_vectors && r / 64 < mask.size(); ++r) {
		const bool w = r < want.size() && want[r]; // (the padding behind n_values never qualifies)
		bad += (((mask[r / 64] >> (r % 64)) & 1) != 0) != w;
		set += w;
	}
	EXPECT(bad == 0, "%s %s: %zu bits differ from a scan of decompress", name, what, bad);
	EXPECT(!want_some || (set > 0 && set < want.size()), "%s %s: the case selects %zu of %zu values", name, what, set, want.size());
	const std::vector<int64_t> idx = alp::gpu::column<double>::mask_indices(mask);
	std::vector<int64_t>       widx;
	for (size_t r = 0; r < want.size(); ++r) {
		if (want[r]) { widx.push_back(static_cast<int64_t>(r)); }
	}
	EXPECT(idx == widx, "%s %s: mask_indices gives %zu indices, a scan %zu, or they differ", name, what, idx.size(), widx.size());
}

template <class PT>
void run(const char* name, size_t n_values, unsigned seed) {
	using column                  = alp::gpu::column<PT>;
	const std::vector<PT>      a  = make_column<PT>(n_values, seed), b = make_column<PT>(n_values, seed + 100), c = make_column<PT>(n_values, seed + 200);
	const std::vector<uint8_t> ba = column::compress(a.data(), a.size()), bb = column::compress(b.data(), b.size()), bc = column::compress(c.data(), c.size());
	const std::vector<PT>      da = column::decompress(ba.data(), ba.size()), db = column::decompress(bb.data(), bb.size()), dc = column::decompress(bc.data(), bc.size());
	const size_t               nv = (n_values + 1023) / 1024;
	const PT lo1 = PT(-2500.5), hi1 = PT(1234.25), lo2 = PT(0.125), hi2 = PT(4000);
	std::vector<bool> qa(n_values), qb(n_values), q_and(n_values), q_or(n_values);
	for (size_t i = 0; i < n_values; ++i) {
		qa[i]    = da[i] >= lo1 && da[i] <= hi1;
		qb[i]    = db[i] >= lo2 && db[i] <= hi2;
		q_and[i] = qa[i] && qb[i];
		q_or[i]  = qa[i] || qb[i];
	}
	const std::vector<uint64_t> ma = column::select_mask(ba.data(), ba.size(), lo1, hi1);
	check_mask(name, "a", ma, qa, nv, true);
	std::vector<uint64_t> m_and = ma, m_or = ma;
	column::select_mask(bb.data(), bb.size(), lo2, hi2, column::mask_and, m_and);
	column::select_mask(bb.data(), bb.size(), lo2, hi2, column::mask_or, m_or);
	check_mask(name, "a AND b", m_and, q_and, nv, true);
	check_mask(name, "a OR b", m_or, q_or, nv, true);
	check_mask(name, "nothing", column::select_mask(ba.data(), ba.size(), PT(5), PT(-5)), std::vector<bool>(n_values, false), nv, false);

	const struct {
		const char*                  what;
		const std::vector<uint64_t>& mask;
		const std::vector<bool>&     bit;
	} sums[] = {{"SUM(c) WHERE a AND b", m_and, q_and}, {"SUM(c) WHERE a OR b", m_or, q_or}};
	for (const auto& s : sums) {
		// (a NaN of c under the mask would make both sides NaN, which compare unequal as bits only by payload: the masks are cleared of them)
		std::vector<uint64_t> mask = s.mask;
		std::vector<bool>     bit  = s.bit;
		for (size_t i = 0; i < n_values; ++i) {
			if (dc[i] != dc[i]) {
				mask[i / 64] &= ~(uint64_t(1) << (i % 64));
				bit[i] = false;
			}
		}
		const auto got  = column::sum_masked(bc.data(), bc.size(), mask);
		const double want = host_sum_masked(dc, bit, nv);
		uint64_t     count = 0, gb, wb;
		for (size_t i = 0; i < n_values; ++i) { count += bit[i]; }
		std::memcpy(&gb, &got.sum, 8);
		std::memcpy(&wb, &want, 8);
		EXPECT(gb == wb, "%s %s: sum %.17g, the host replica of the documented order gives %.17g", name, s.what, got.sum, want);
		EXPECT(got.count == count && count > 0, "%s %s: count %llu, expected %llu", name, s.what, (unsigned long long)got.count, (unsigned long long)count);
	}
	bool threw = false;
	try {
		std::vector<uint64_t> shorter(ma.begin(), ma.end() - 16);
		column::select_mask(bb.data(), bb.size(), lo2, hi2, column::mask_and, shorter);
	} catch (const std::exception&) { threw = true; }
	EXPECT(threw, "%s: a mask of the wrong length did not throw", name);
	threw = false;
	try {
		column::sum_masked(bc.data(), bc.size(), std::vector<uint64_t>(16 * nv + 16));
	} catch (const std::exception&) { threw = true; }
	EXPECT(threw, "%s: sum_masked with a mask of the wrong length did not throw", name);
	std::printf("%s: %zu values\n", name, n_values);
}

int main() {
	run<double>("double", 250 * 1024 + 333, 5);
	run<float>("float", 230 * 1024 + 77, 6);
	std::printf("mask_test: %d failures\n", failures);
	return failures ? 1 : 0;
}
