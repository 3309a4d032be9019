// top_k_test.cpp — alp::gpu::column<PT>::top_k (include/alp/batch.hpp; include/alpgpu.h, "top-k") on a serialized column read from a file, against
// column::decompress and a host std::partial_sort with the comparator of the definition, bit for bit:
//   top_k_test f64|f32 col.blob in.mask
// Prints "ok <vectors> <selected values that are no NaNs>" and returns 0 when everything agrees; tests/test_top_k_gpu.py builds and runs it.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/top_k_test.cpp -Lalp_amd -lalpgpu -ldl
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
	std::vector<int64_t> selected;
	for (uint64_t r = 0; r < x.size(); ++r) {
		if (((mask[r >> 6] >> (r & 63)) & 1ull) && !std::isnan(x[r])) { selected.push_back(static_cast<int64_t>(r)); }
	}
	const std::vector<typename column::zone> records = column::minmax_masked(blob.data(), blob.size(), mask);
	const uint64_t                           ks[]    = {0, 1, 7, 100, 1024};
	for (const bool largest : {true, false}) {
		const auto before = [&](int64_t a, int64_t b) {
			const uint64_t ka = order_key(x[a]), kb = order_key(x[b]);
			return ka != kb ? (largest ? ka > kb : ka < kb) : a < b;
		};
		for (const uint64_t k : ks) {
			std::vector<int64_t> want = selected;
			const size_t         n    = std::min<size_t>(k, want.size());
			std::partial_sort(want.begin(), want.begin() + n, want.end(), before);
			want.resize(n);
			for (const bool with_records : {false, true}) {
				const typename column::top_k_result got = column::top_k(blob.data(), blob.size(), mask, k, largest, with_records ? &records : nullptr);
				bool                                same = got.indices == want && got.values.size() == n;
				for (size_t j = 0; same && j < n; ++j) { same = std::memcmp(&got.values[j], &x[want[j]], sizeof(PT)) == 0; }
				if (!same) {
					std::printf("FAIL: top_k, k %llu, largest %d, records %d: %zu results for %zu\n", static_cast<unsigned long long>(k), int(largest), int(with_records), got.indices.size(), n);
					return 1;
				}
			}
		}
	}
	// a mask of the wrong length, a k beyond the bound and records of the wrong length throw
	int threw = 0;
	try {
		column::top_k(blob.data(), blob.size(), std::vector<uint64_t>(mask.size() + 16), 10);
	} catch (const std::exception&) { ++threw; }
	try {
		column::top_k(blob.data(), blob.size(), mask, ALPGPU_TOP_K_MAX + 1);
	} catch (const std::exception&) { ++threw; }
	try {
		const std::vector<typename column::zone> few(records.begin(), records.end() - 1);
		column::top_k(blob.data(), blob.size(), mask, 10, true, &few);
	} catch (const std::exception&) { ++threw; }
	if (threw != 3) {
		std::printf("FAIL: %d of 3 misuses threw\n", threw);
		return 1;
	}
	std::printf("ok %llu %zu\n", static_cast<unsigned long long>(nv), selected.size());
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 4) {
		std::printf("usage: top_k_test f64|f32 col.blob in.mask\n");
		return 2;
	}
	try {
		return std::strcmp(argv[1], "f32") == 0 ? run<float>(argv) : run<double>(argv);
	} catch (const std::exception& e) {
		std::printf("FAIL: %s\n", e.what());
		return 1;
	}
}
