// take_test.cpp — alp::gpu::column<PT>::take (include/alp/batch.hpp): values of a serialized column at value indices, gathered on the GPU where they
// lie (include/alpgpu.h: alpgpu_gather_*), against alp::gpu::column<PT>::decompress of the same blob, bit for bit.  Double and float columns with ALP
// and ALP_RD rowgroups, exceptions and specials and an incomplete last vector; indices in any order, repeated, in the tail padding and past the
// end (the canonical quiet NaN); an empty index list; a blob too short for its header throws.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/take_test.cpp -Lalp_amd -lalpgpu && ./a.out
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

template <class PT, class U>
void run(const char* name, size_t n_values, unsigned seed) {
	const std::vector<PT>      col  = make_column<PT>(n_values, seed);
	const std::vector<uint8_t> blob = alp::gpu::column<PT>::compress(col.data(), col.size());
	const std::vector<PT>      all  = alp::gpu::column<PT>::decompress(blob.data(), blob.size());
	const uint64_t             n_padded = (n_values + 1023) / 1024 * 1024;
	std::mt19937_64            rng(seed + 1);
	std::vector<uint64_t>      idx;
	for (int i = 0; i < 20000; ++i) { idx.push_back(rng() % n_values); }
	for (uint64_t i = 0; i < n_values; i += 997) { idx.push_back(i); }
	idx.push_back(n_values - 1);
	idx.push_back(idx[5]);
	const size_t n_in = idx.size();
	for (uint64_t i = n_values; i < n_padded; i += 101) { idx.push_back(i); } // tail padding: a value of the column's last vector
	idx.push_back(n_padded);                                                  // past the end
	idx.push_back(~uint64_t(0));
	const std::vector<PT> got = alp::gpu::column<PT>::take(blob.data(), blob.size(), idx.data(), idx.size());
	EXPECT(got.size() == idx.size(), "%s: %zu values for %zu indices", name, got.size(), idx.size());
	size_t bad = 0;
	for (size_t k = 0; k < n_in && k < got.size(); ++k) {
		U a, b;
		std::memcpy(&a, &got[k], sizeof(U));
		std::memcpy(&b, &all[idx[k]], sizeof(U));
		bad += a != b;
		std::memcpy(&b, &col[idx[k]], sizeof(U));
		bad += a != b;
	}
	EXPECT(bad == 0, "%s: %zu values differ from decompress / the input", name, bad);
	const U nan_bits = sizeof(U) == 8 ? U(0x7FF8000000000000ull) : U(0x7FC00000u);
	for (size_t k = idx.size() - 2; k < got.size(); ++k) {
		U a;
		std::memcpy(&a, &got[k], sizeof(U));
		EXPECT(a == nan_bits, "%s: index %llu past the end did not give the canonical NaN", name, static_cast<unsigned long long>(idx[k]));
	}
	U pad; // the tail padding repeats the first value of the incomplete last vector (alpgpu_pad_tail_*)
	std::memcpy(&pad, &col[n_values / 1024 * 1024], sizeof(U));
	for (size_t k = n_in; k + 2 < got.size(); ++k) {
		U a;
		std::memcpy(&a, &got[k], sizeof(U));
		EXPECT(a == pad, "%s: tail padding index %llu is not the padding value", name, static_cast<unsigned long long>(idx[k]));
	}
	EXPECT(alp::gpu::column<PT>::take(blob.data(), blob.size(), idx.data(), 0).empty(), "%s: no indices, no values", name);
	bool threw = false;
	try {
		alp::gpu::column<PT>::take(blob.data(), 40, idx.data(), 4);
	} catch (const std::exception&) { threw = true; }
	EXPECT(threw, "%s: a blob shorter than its header did not throw", name);
	std::printf("%s: %zu values, %zu indices\n", name, n_values, idx.size());
}

int main() {
	run<double, uint64_t>("double", 250 * 1024 + 333, 5);
	run<float, uint32_t>("float", 230 * 1024 + 77, 6);
	std::printf("take_test: %d failures\n", failures);
	return failures ? 1 : 0;
}
