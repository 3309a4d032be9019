// in_list_test.cpp — alp::gpu::column<PT>::select_in_mask (include/alp/batch.hpp; include/alpgpu.h, "set membership") on a serialized column read
// from a file, against column::decompress and a host loop over the definition of a member (some element == the value), bit for bit:
//   in_list_test f64|f32 col.blob values.bin in.mask
// values.bin holds the list in the column's type, in any order (the wrapper sorts); in.mask is a prior bitmap for the combining forms.  Prints
// "ok <vectors> <members>" and returns 0 when everything agrees; tests/test_in_list_gpu.py builds and runs it.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/in_list_test.cpp -Lalp_amd -lalpgpu -ldl
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
	const std::vector<uint8_t> blob = read_file(argv[2]), raw_values = read_file(argv[3]), raw_mask = read_file(argv[4]);
	std::vector<PT>            values(raw_values.size() / sizeof(PT));
	std::memcpy(values.data(), raw_values.data(), values.size() * sizeof(PT));
	std::vector<uint64_t> prior(raw_mask.size() / sizeof(uint64_t));
	std::memcpy(prior.data(), raw_mask.data(), prior.size() * sizeof(uint64_t));
	const std::vector<PT> x = column::decompress(blob.data(), blob.size());
	if (x.size() % 1024 != 0 || prior.size() != x.size() / 64) {
		std::printf("FAIL: %zu values, %zu mask words\n", x.size(), prior.size());
		return 1;
	}
	// the definition, word by word
	std::vector<uint64_t> member(prior.size(), 0);
	uint64_t              n_members = 0;
	for (uint64_t r = 0; r < x.size(); ++r) {
		bool m = false;
		for (const PT e : values) { m = m || e == x[r]; }
		if (m) {
			member[r >> 6] |= 1ull << (r & 63);
			++n_members;
		}
	}
	const auto same = [&](const std::vector<uint64_t>& got, const char* what, auto&& want) {
		if (got.size() != prior.size()) {
			std::printf("FAIL: %s returned %zu words\n", what, got.size());
			return false;
		}
		for (uint64_t w = 0; w < got.size(); ++w) {
			if (got[w] != want(w)) {
				std::printf("FAIL: %s, word %llu\n", what, static_cast<unsigned long long>(w));
				return false;
			}
		}
		return true;
	};
	if (!same(column::select_in_mask(blob.data(), blob.size(), values), "select_in_mask", [&](uint64_t w) { return member[w]; })) { return 1; }
	if (!same(column::select_in_mask(blob.data(), blob.size(), values, true), "select_in_mask negated", [&](uint64_t w) { return ~member[w]; })) { return 1; }
	if (!same(column::select_in_mask(blob.data(), blob.size(), std::vector<PT>()), "select_in_mask of nothing", [&](uint64_t) { return 0ull; })) { return 1; }
	std::vector<uint64_t> m = prior;
	column::select_in_mask(blob.data(), blob.size(), values, false, column::mask_and, m);
	if (!same(m, "select_in_mask AND", [&](uint64_t w) { return prior[w] & member[w]; })) { return 1; }
	m = prior;
	column::select_in_mask(blob.data(), blob.size(), values, true, column::mask_or, m);
	if (!same(m, "select_in_mask OR negated", [&](uint64_t w) { return prior[w] | ~member[w]; })) { return 1; }
	m = prior;
	column::select_in_mask(blob.data(), blob.size(), values, false, column::mask_set, m);
	if (!same(m, "select_in_mask SET into a mask", [&](uint64_t w) { return member[w]; })) { return 1; }
	bool threw = false;
	try {
		std::vector<uint64_t> bad(prior.size() + 1, 0);
		column::select_in_mask(blob.data(), blob.size(), values, false, column::mask_and, bad);
	} catch (const std::runtime_error&) { threw = true; }
	if (!threw) {
		std::printf("FAIL: a mask of the wrong length was accepted\n");
		return 1;
	}
	std::printf("ok %zu %llu\n", x.size() / 1024, static_cast<unsigned long long>(n_members));
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 5) {
		std::printf("usage: in_list_test f64|f32 col.blob values.bin in.mask\n");
		return 2;
	}
	try {
		return std::string(argv[1]) == "f32" ? run<float>(argv) : run<double>(argv);
	} catch (const std::exception& e) {
		std::printf("FAIL: %s\n", e.what());
		return 1;
	}
}
