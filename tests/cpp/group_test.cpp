// group_test.cpp — alp::gpu::column<PT>::group_sum_masked / group_totals (include/alp/batch.hpp; include/alpgpu.h, "grouped aggregation") on two
// serialized columns read from files, for tests/test_group_gpu.py to compare byte for byte with what the Python route gives for the same blobs:
//   group_test f64|f32 val.blob key.blob in.mask bounds.bin sums.bin counts.bin
// bounds.bin holds n_groups lower bounds and then n_groups upper bounds in the columns' type; sums.bin and counts.bin receive the
// [n_groups][n_vectors] results, and every group's total is printed as "total <g> <bits of the sum as 16 hex digits> <count>".
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/group_test.cpp -Lalp_amd -lalpgpu -ldl
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

template <class T>
static void write_file(const char* path, const std::vector<T>& v) {
	std::ofstream out(path, std::ios::binary);
	out.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
	if (!out) { throw std::runtime_error(std::string("cannot write ") + path); }
}

template <class PT>
static int run(char** argv) {
	using column                     = alp::gpu::column<PT>;
	const std::vector<uint8_t> val = read_file(argv[2]), key = read_file(argv[3]), raw_mask = read_file(argv[4]), raw_bounds = read_file(argv[5]);
	std::vector<uint64_t>      mask(raw_mask.size() / sizeof(uint64_t));
	std::memcpy(mask.data(), raw_mask.data(), mask.size() * sizeof(uint64_t));
	std::vector<PT> bounds(raw_bounds.size() / sizeof(PT));
	std::memcpy(bounds.data(), raw_bounds.data(), bounds.size() * sizeof(PT));
	const uint32_t n_groups = static_cast<uint32_t>(bounds.size() / 2);
	const PT *     lo = bounds.data(), *hi = bounds.data() + n_groups;
	std::vector<double>   sums;
	std::vector<uint32_t> counts;
	const uint64_t        nv = column::group_sum_masked(val.data(), val.size(), key.data(), key.size(), mask, lo, hi, n_groups, sums, &counts);
	write_file(argv[6], sums);
	write_file(argv[7], counts);
	const auto totals = column::group_totals(sums, &counts, nv, n_groups);
	for (uint32_t g = 0; g < n_groups; ++g) {
		uint64_t bits;
		std::memcpy(&bits, &totals[g].sum, sizeof(bits));
		std::printf("total %u %016llx %llu\n", g, static_cast<unsigned long long>(bits), static_cast<unsigned long long>(totals[g].count));
	}
	// without counts the sums are the same
	std::vector<double> again;
	column::group_sum_masked(val.data(), val.size(), key.data(), key.size(), mask, lo, hi, n_groups, again);
	if (again.size() != sums.size() || std::memcmp(again.data(), sums.data(), sums.size() * sizeof(double)) != 0) {
		std::printf("FAIL: the sums without counts differ\n");
		return 1;
	}
	// a mask of the wrong length, no group, too many groups, and sums of the wrong shape, throw
	int threw = 0;
	try {
		column::group_sum_masked(val.data(), val.size(), key.data(), key.size(), std::vector<uint64_t>(mask.size() + 16), lo, hi, n_groups, again);
	} catch (const std::exception&) { ++threw; }
	try {
		column::group_sum_masked(val.data(), val.size(), key.data(), key.size(), mask, lo, hi, 0, again);
	} catch (const std::exception&) { ++threw; }
	try {
		const std::vector<PT> many(ALPGPU_GROUP_MAX + 1, PT(0));
		column::group_sum_masked(val.data(), val.size(), key.data(), key.size(), mask, many.data(), many.data(), ALPGPU_GROUP_MAX + 1, again);
	} catch (const std::exception&) { ++threw; }
	try {
		column::group_totals(sums, &counts, nv + 1, n_groups);
	} catch (const std::exception&) { ++threw; }
	if (threw != 4) {
		std::printf("FAIL: %d of 4 misuses threw\n", threw);
		return 1;
	}
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 8) {
		std::printf("usage: group_test f64|f32 val.blob key.blob in.mask bounds.bin sums.bin counts.bin\n");
		return 2;
	}
	try {
		return std::strcmp(argv[1], "f32") == 0 ? run<float>(argv) : run<double>(argv);
	} catch (const std::exception& e) {
		std::printf("FAIL: %s\n", e.what());
		return 1;
	}
}
