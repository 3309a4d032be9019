// quantile_test.cpp — alp::gpu::column<PT>::select_rank and ::quantile (include/alp/batch.hpp; include/alpgpu.h, "quantiles") on a serialized column read
// from a file, against column::decompress and a host std::sort with the comparator of the definition, bit for bit:
//   quantile_test f64|f32 col.blob in.mask
// Prints "ok <vectors> <selected values that are no NaNs>" and returns 0 when everything agrees; tests/test_quantile_gpu.py builds and runs it.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/quantile_test.cpp -Lalp_amd -lalpgpu -ldl
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "alp.hpp"
#include "alp/batch.hpp"

static std::vector<uint8_t> read_file(const char* path) {
	std::ifstream in(path, std::ios::binary);
	if (!in) { throw std::runtime_error(std::string("cannot read ") + path); }
	return std::vector<uint8_t>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

// okey of the definition: bits ^ (sign ? all-ones : sign-bit), unsigned
template <class PT>
static uint64_t order_key(PT x) {
	typename std::conditional<sizeof(PT) == 8, uint64_t, uint32_t>::type b;
	std::memcpy(&b, &x, sizeof(b));
	const decltype(b) sign = static_cast<decltype(b)>(1) << (8 * sizeof(b) - 1);
	return b & sign ? static_cast<decltype(b)>(~b) : static_cast<decltype(b)>(b | sign);
}

template <class PT>
static bool same_bits(const std::vector<PT>& a, const std::vector<PT>& b) {
	return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(PT)) == 0);
}

template <class PT>
static int run(char** argv) {
	using column = alp::gpu::column<PT>;
	const std::vector<uint8_t> blob = read_file(argv[2]), raw_mask = read_file(argv[3]);
	std::vector<uint64_t>      mask(raw_mask.size() / sizeof(uint64_t));
	std::memcpy(mask.data(), raw_mask.data(), mask.size() * sizeof(uint64_t));
	const std::vector<PT> x  = column::decompress(blob.data(), blob.size());
	const uint64_t        nv = mask.size() / 16;
	if (x.size() != nv * 1024) {
		std::printf("FAIL: %zu values, %zu mask words\n", x.size(), mask.size());
		return 1;
	}
	std::vector<PT> s;
	for (uint64_t r = 0; r < x.size(); ++r) {
		if (((mask[r >> 6] >> (r & 63)) & 1ull) && !std::isnan(x[r])) { s.push_back(x[r]); }
	}
	std::sort(s.begin(), s.end(), [](PT a, PT b) { return order_key(a) < order_key(b); });
	const uint64_t n = s.size();
	if (n == 0) {
		std::printf("FAIL: the mask selects no number\n");
		return 1;
	}
	const std::vector<typename column::zone> masked = column::minmax_masked(blob.data(), blob.size(), mask), whole = column::zone_map(blob.data(), blob.size());
	const std::vector<std::vector<uint64_t>> rank_sets = {{0}, {n - 1}, {n / 2, 3, n / 2, n + 7, ~0ull, 1}, {}};
	std::vector<uint64_t>                    many;
	for (uint64_t i = 0; i < ALPGPU_RANK_MAX; ++i) { many.push_back((n - 1) * i / (ALPGPU_RANK_MAX - 1)); }
	for (const bool from_top : {false, true}) {
		for (std::vector<uint64_t> ranks : rank_sets) {
			if (ranks.empty()) { ranks = many; }
			std::vector<PT> want;
			for (const uint64_t r : ranks) {
				const uint64_t at = std::min(r, n - 1);
				want.push_back(s[from_top ? n - 1 - at : at]);
			}
			for (const std::vector<typename column::zone>* zones : {static_cast<const std::vector<typename column::zone>*>(nullptr), &masked, &whole}) {
				const typename column::quantile_result got = column::select_rank(blob.data(), blob.size(), mask, ranks, from_top, zones);
				if (got.count != n || !same_bits(got.lower, want) || !got.upper.empty() || !got.ranks.empty()) {
					std::printf("FAIL: select_rank, %zu ranks, from_top %d, zones %d: count %llu for %llu\n", ranks.size(), int(from_top), int(zones != nullptr),
					            static_cast<unsigned long long>(got.count), static_cast<unsigned long long>(n));
					return 1;
				}
			}
		}
	}
	const std::vector<std::vector<double>> q_sets = {{0.5}, {0.0, 0.25, 0.5, 0.75, 1.0}, {1.0, 0.999, 0.5, 0.5, 0.001, 0.0, 0.3, 0.3, 0.9, 0.1, 0.2, 0.6, 0.7, 0.8, 0.4, 0.05}};
	for (const std::vector<double>& q : q_sets) {
		std::vector<PT>       lower, upper;
		std::vector<uint64_t> ranks;
		for (const double qi : q) {
			const volatile double pos = qi * static_cast<double>(n - 1); // one multiplication, not fused with anything
			const uint64_t        r   = std::min<uint64_t>(n - 1, static_cast<uint64_t>(std::floor(pos)));
			ranks.push_back(r);
			lower.push_back(s[r]);
			upper.push_back(s[std::min(r + 1, n - 1)]);
		}
		for (const std::vector<typename column::zone>* zones : {static_cast<const std::vector<typename column::zone>*>(nullptr), &masked, &whole}) {
			const typename column::quantile_result got = column::quantile(blob.data(), blob.size(), mask, q, zones);
			if (got.count != n || !same_bits(got.lower, lower) || !same_bits(got.upper, upper) || got.ranks != ranks) {
				std::printf("FAIL: quantile, %zu quantiles, zones %d: count %llu for %llu\n", q.size(), int(zones != nullptr), static_cast<unsigned long long>(got.count),
				            static_cast<unsigned long long>(n));
				return 1;
			}
		}
	}
	// an empty selection: the count and nothing else
	const typename column::quantile_result none = column::quantile(blob.data(), blob.size(), std::vector<uint64_t>(mask.size(), 0), {0.5});
	if (none.count != 0 || !none.lower.empty() || !none.upper.empty() || !none.ranks.empty()) {
		std::printf("FAIL: an empty selection gave something\n");
		return 1;
	}
	// a mask of the wrong length, too many or no ranks, a quantile outside [0, 1] and records of the wrong length throw
	int        threw = 0;
	const auto must_throw = [&](auto&& call) {
		try {
			call();
		} catch (const std::exception&) { ++threw; }
	};
	must_throw([&] { column::select_rank(blob.data(), blob.size(), std::vector<uint64_t>(mask.size() + 16), {1}); });
	must_throw([&] { column::select_rank(blob.data(), blob.size(), mask, std::vector<uint64_t>(ALPGPU_RANK_MAX + 1, 0)); });
	must_throw([&] { column::select_rank(blob.data(), blob.size(), mask, {}); });
	must_throw([&] { column::quantile(blob.data(), blob.size(), mask, std::vector<double>(ALPGPU_QUANTILE_MAX + 1, 0.5)); });
	must_throw([&] { column::quantile(blob.data(), blob.size(), mask, {0.5, 1.5}); });
	must_throw([&] { column::quantile(blob.data(), blob.size(), mask, {std::nan("")}); });
	must_throw([&] {
		const std::vector<typename column::zone> few(masked.begin(), masked.end() - 1);
		column::quantile(blob.data(), blob.size(), mask, {0.5}, &few);
	});
	if (threw != 7) {
		std::printf("FAIL: %d of 7 misuses threw\n", threw);
		return 1;
	}
	std::printf("ok %llu %llu\n", static_cast<unsigned long long>(nv), static_cast<unsigned long long>(n));
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 4) {
		std::printf("usage: quantile_test f64|f32 col.blob in.mask\n");
		return 2;
	}
	try {
		return std::strcmp(argv[1], "f32") == 0 ? run<float>(argv) : run<double>(argv);
	} catch (const std::exception& e) {
		std::printf("FAIL: %s\n", e.what());
		return 1;
	}
}
