// pair_test.cpp — alp::gpu::column<PT>::compare_mask / dot_masked (include/alp/batch.hpp; include/alpgpu.h, "two-column consumers") on two
// serialized columns read from files, for tests/test_pair_gpu.py to compare byte for byte with what the Python route gives for the same blobs:
//   pair_test f64|f32 a.blob b.blob prior.mask set.mask and.mask
// writes compare_mask(a, b, cmp_le) to set.mask, compare_mask(a, b, cmp_gt, mask_and) over prior.mask to and.mask, and prints
// "dot <bits of the sum as 16 hex digits> <count>" for dot_masked(a, b) under and.mask.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/pair_test.cpp -Lalp_amd -lalpgpu -ldl
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

static void write_mask(const char* path, const std::vector<uint64_t>& mask) {
	std::ofstream out(path, std::ios::binary);
	out.write(reinterpret_cast<const char*>(mask.data()), static_cast<std::streamsize>(mask.size() * sizeof(uint64_t)));
	if (!out) { throw std::runtime_error(std::string("cannot write ") + path); }
}

template <class PT>
static int run(char** argv) {
	using column                     = alp::gpu::column<PT>;
	const std::vector<uint8_t> a     = read_file(argv[2]), b = read_file(argv[3]), prior = read_file(argv[4]);
	const std::vector<uint64_t> fresh = column::compare_mask(a.data(), a.size(), b.data(), b.size(), column::cmp_le);
	write_mask(argv[5], fresh);
	std::vector<uint64_t> mask(prior.size() / sizeof(uint64_t));
	std::memcpy(mask.data(), prior.data(), mask.size() * sizeof(uint64_t));
	column::compare_mask(a.data(), a.size(), b.data(), b.size(), column::cmp_gt, column::mask_and, mask);
	write_mask(argv[6], mask);
	const auto dot = column::dot_masked(a.data(), a.size(), b.data(), b.size(), mask);
	uint64_t   bits;
	std::memcpy(&bits, &dot.sum, sizeof(bits));
	std::printf("dot %016llx %llu\n", static_cast<unsigned long long>(bits), static_cast<unsigned long long>(dot.count));
	// a mask of the wrong length, and columns of different lengths, throw
	int threw = 0;
	try {
		std::vector<uint64_t> shorter(mask.begin(), mask.end() - 16);
		column::compare_mask(a.data(), a.size(), b.data(), b.size(), column::cmp_gt, column::mask_and, shorter);
	} catch (const std::exception&) { ++threw; }
	try {
		column::dot_masked(a.data(), a.size(), b.data(), b.size(), std::vector<uint64_t>(mask.size() + 16));
	} catch (const std::exception&) { ++threw; }
	try {
		const std::vector<PT>      few(1024, PT(1));
		const std::vector<uint8_t> c = column::compress(few.data(), few.size());
		column::compare_mask(a.data(), a.size(), c.data(), c.size(), column::cmp_eq);
	} catch (const std::exception&) { ++threw; }
	if (threw != 3) {
		std::printf("FAIL: %d of 3 misuses threw\n", threw);
		return 1;
	}
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 7) {
		std::printf("usage: pair_test f64|f32 a.blob b.blob prior.mask set.mask and.mask\n");
		return 2;
	}
	try {
		return std::strcmp(argv[1], "f32") == 0 ? run<float>(argv) : run<double>(argv);
	} catch (const std::exception& e) {
		std::printf("FAIL: %s\n", e.what());
		return 1;
	}
}
