// take_masked_test.cpp — alp::gpu::column<PT>::take_masked (include/alp/batch.hpp; include/alpgpu.h, "masked projection") against a host-side
// filter of alp::gpu::column<PT>::decompress of the same blobs: SELECT c WHERE p(a) AND q(b) with the bitmap made by select_mask + mask_and,
// the values compared as bit patterns (NaN payloads and the sign of -0.0 included), the indices against a scan of the predicate and against
// mask_indices.  Double and float columns with ALP and ALP_RD rowgroups, exceptions, specials and an incomplete last vector.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/take_masked_test.cpp -Lalp_amd -lalpgpu -ldl && ./a.out
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

template <class PT>
static bool same_bits(const std::vector<PT>& x, const std::vector<PT>& y) {
	return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(PT)) == 0);
}

template <class PT>
void run(const char* name, size_t n_values, unsigned seed) {
	using column                  = alp::gpu::column<PT>;
	const std::vector<PT>      a  = make_column<PT>(n_values, seed), b = make_column<PT>(n_values, seed + 100), c = make_column<PT>(n_values, seed + 200);
	const std::vector<uint8_t> ba = column::compress(a.data(), a.size()), bb = column::compress(b.data(), b.size()), bc = column::compress(c.data(), c.size());
	const std::vector<PT>      da = column::decompress(ba.data(), ba.size()), db = column::decompress(bb.data(), bb.size()), dc = column::decompress(bc.data(), bc.size());
	const size_t               nv = (n_values + 1023) / 1024;
	const PT lo1 = PT(-2500.5), hi1 = PT(1234.25), lo2 = PT(-3000.75), hi2 = PT(4000);

	std::vector<uint64_t> mask = column::select_mask(ba.data(), ba.size(), lo1, hi1);
	column::select_mask(bb.data(), bb.size(), lo2, hi2, column::mask_and, mask);
	std::vector<int64_t> widx;
	std::vector<PT>      wc, wa;
	size_t               specials = 0;
	for (size_t i = 0; i < n_values; ++i) {
		if (da[i] >= lo1 && da[i] <= hi1 && db[i] >= lo2 && db[i] <= hi2) {
			widx.push_back(static_cast<int64_t>(i));
			wc.push_back(dc[i]);
			wa.push_back(da[i]);
			specials += dc[i] != dc[i] || (dc[i] == 0 && std::signbit(dc[i]));
		}
	}
	EXPECT(!widx.empty() && widx.size() < n_values, "%s: the predicates select %zu of %zu values", name, widx.size(), n_values);
	EXPECT(specials > 0, "%s: no NaN and no -0.0 of c is selected: the case does not test their bits", name);

	std::vector<int64_t>  idx {-1, -2};
	const std::vector<PT> vals = column::take_masked(bc.data(), bc.size(), mask), vals2 = column::take_masked(bc.data(), bc.size(), mask, idx);
	EXPECT(same_bits(vals, wc), "%s: take_masked(c) gives %zu values, a filter of decompress %zu, or their bits differ", name, vals.size(), wc.size());
	EXPECT(same_bits(vals2, wc), "%s: take_masked(c, indices) differs from a filter of decompress", name);
	EXPECT(idx == widx, "%s: take_masked's indices (%zu) differ from a scan of the predicates (%zu)", name, idx.size(), widx.size());
	EXPECT(idx == column::mask_indices(mask), "%s: take_masked's indices differ from mask_indices", name);
	EXPECT(same_bits(column::take_masked(ba.data(), ba.size(), mask), wa), "%s: take_masked(a) differs from a filter of decompress", name);

	// an empty and a full bitmap; the padding behind n_values is the caller's to keep out, so "full" stops at n_values
	std::vector<uint64_t> none(16 * nv, 0), all(16 * nv, 0);
	for (size_t i = 0; i < n_values; ++i) { all[i / 64] |= uint64_t(1) << (i % 64); }
	idx.assign(3, 7);
	EXPECT(column::take_masked(bc.data(), bc.size(), none, idx).empty() && idx.empty(), "%s: an empty bitmap selected something", name);
	EXPECT(same_bits(column::take_masked(bc.data(), bc.size(), all), dc), "%s: a full bitmap does not give decompress", name);

	bool threw = false;
	try {
		column::take_masked(bc.data(), bc.size(), std::vector<uint64_t>(16 * nv + 16));
	} catch (const std::exception&) { threw = true; }
	EXPECT(threw, "%s: take_masked with a mask of the wrong length did not throw", name);
	std::printf("%s: %zu values, %zu selected\n", name, n_values, widx.size());
}

int main() {
	run<double>("double", 250 * 1024 + 333, 5);
	run<float>("float", 230 * 1024 + 77, 6);
	std::printf("take_masked_test: %d failures\n", failures);
	return failures ? 1 : 0;
}
