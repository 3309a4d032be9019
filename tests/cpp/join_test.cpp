// join_test.cpp — alp::gpu::column<PT>::join_probe (include/alp/batch.hpp; include/alpgpu.h, "join probe") on a serialized column read from a file,
// against column::decompress and a host loop over the definition (span = the keys == the value, pos = a key that is, the first of them in `keys`):
//   join_test f64|f32 col.blob keys.bin in.mask
// keys.bin holds the keys in the column's type, in any order (the wrapper sorts, stably, and maps positions back); in.mask is a bitmap.  Prints
// "ok <vectors> <rows under the mask> <matched rows under the mask>" and returns 0 when everything agrees; tests/test_join_probe_gpu.py builds and runs it.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/join_test.cpp -Lalp_amd -lalpgpu -ldl
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "alp.hpp"
#include "alp/batch.hpp"

static std::vector<uint8_t> read_file(const char* path) {
	std::ifstream in(path, std::ios::binary);
	if (!in) { throw std::runtime_error(std::string("cannot read ") + path); }
	return std::vector<uint8_t>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

template <class PT>
static int run(char** argv) {
	using column = alp::gpu::column<PT>;
	const std::vector<uint8_t> blob = read_file(argv[2]), raw_keys = read_file(argv[3]), raw_mask = read_file(argv[4]);
	std::vector<PT>            keys(raw_keys.size() / sizeof(PT));
	std::memcpy(keys.data(), raw_keys.data(), keys.size() * sizeof(PT));
	std::vector<uint64_t> mask(raw_mask.size() / sizeof(uint64_t));
	std::memcpy(mask.data(), raw_mask.data(), mask.size() * sizeof(uint64_t));
	const std::vector<PT> x = column::decompress(blob.data(), blob.size());
	if (x.size() % 1024 != 0 || mask.size() != x.size() / 64) {
		std::printf("FAIL: %zu values, %zu mask words\n", x.size(), mask.size());
		return 1;
	}
	// the definition, value by value
	std::vector<int64_t>  first_eq(x.size(), ALPGPU_JOIN_NO_MATCH);
	std::vector<uint32_t> n_eq(x.size(), 0);
	for (uint64_t r = 0; r < x.size(); ++r) {
		for (size_t k = 0; k < keys.size(); ++k) {
			if (keys[k] == x[r]) {
				if (n_eq[r]++ == 0) { first_eq[r] = static_cast<int64_t>(k); }
			}
		}
	}
	uint64_t   n_rows = 0, n_matched = 0;
	const auto check = [&](const typename column::join_result& got, const std::vector<uint64_t>* m, const std::vector<PT>& ks, const char* what, bool tally) {
		uint64_t j = 0;
		for (uint64_t r = 0; r < x.size(); ++r) {
			if (m && !((*m)[r >> 6] >> (r & 63) & 1ull)) { continue; }
			if (j >= got.pos.size() || got.indices.size() != got.pos.size() || got.span.size() != got.pos.size()) {
				std::printf("FAIL: %s returned %zu rows\n", what, got.pos.size());
				return false;
			}
			const int64_t  want_pos  = ks.empty() ? ALPGPU_JOIN_NO_MATCH : first_eq[r];
			const uint32_t want_span = ks.empty() ? 0u : n_eq[r];
			if (got.indices[j] != static_cast<int64_t>(r) || got.pos[j] != want_pos || got.span[j] != want_span) {
				std::printf("FAIL: %s, row %llu (index %llu): pos %lld span %u, expected %lld %u\n", what, static_cast<unsigned long long>(j), static_cast<unsigned long long>(r),
				            static_cast<long long>(got.pos[j]), got.span[j], static_cast<long long>(want_pos), want_span);
				return false;
			}
			if (tally) {
				++n_rows;
				n_matched += want_span > 0 ? 1 : 0;
			}
			++j;
		}
		if (j != got.pos.size()) {
			std::printf("FAIL: %s returned %zu rows, expected %llu\n", what, got.pos.size(), static_cast<unsigned long long>(j));
			return false;
		}
		return true;
	};
	if (!check(column::join_probe(blob.data(), blob.size(), keys, &mask), &mask, keys, "join_probe under the mask", true)) { return 1; }
	if (!check(column::join_probe(blob.data(), blob.size(), keys), nullptr, keys, "join_probe of every value", false)) { return 1; }
	const std::vector<PT> none;
	if (!check(column::join_probe(blob.data(), blob.size(), none, &mask), &mask, none, "join_probe against no keys", false)) { return 1; }
	const std::vector<typename column::zone> zones = column::zone_map(blob.data(), blob.size());
	if (!check(column::join_probe(blob.data(), blob.size(), keys, &mask, &zones), &mask, keys, "join_probe with zones", false)) { return 1; }
	bool threw = false;
	try {
		std::vector<uint64_t> bad(mask.size() + 1, 0);
		column::join_probe(blob.data(), blob.size(), keys, &bad);
	} catch (const std::runtime_error&) { threw = true; }
	if (!threw) {
		std::printf("FAIL: a mask of the wrong length was accepted\n");
		return 1;
	}
	std::printf("ok %zu %llu %llu\n", x.size() / 1024, static_cast<unsigned long long>(n_rows), static_cast<unsigned long long>(n_matched));
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 5) {
		std::printf("usage: join_test f64|f32 col.blob keys.bin in.mask\n");
		return 2;
	}
	try {
		return std::string(argv[1]) == "f32" ? run<float>(argv) : run<double>(argv);
	} catch (const std::exception& e) {
		std::printf("FAIL: %s\n", e.what());
		return 1;
	}
}
