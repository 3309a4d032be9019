// histogram_test.cpp — alp::gpu::column<PT>::histogram (include/alp/batch.hpp; include/alpgpu.h, "histograms") on a serialized column read from a file,
// against column::decompress and a host loop over the definition of a bucket:
//   histogram_test f64|f32 col.blob edges.bin in.mask
// Prints "ok <vectors> <selected values>" and returns 0 when everything agrees; tests/test_histogram_gpu.py builds and runs it.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/histogram_test.cpp -Lalp_amd -lalpgpu -ldl
#include <cmath>
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

// the definition: bucket = the number of edges <= x (right: < x), in whatever order the edges come; a NaN edge is never <= anything
template <class PT>
static std::vector<uint64_t> host_histogram(const std::vector<PT>& x, const std::vector<PT>& edges, const std::vector<uint64_t>* mask, bool right) {
	std::vector<uint64_t> counts(edges.size() + 2, 0);
	for (uint64_t r = 0; r < x.size(); ++r) {
		if (mask && !(((*mask)[r >> 6] >> (r & 63)) & 1ull)) { continue; }
		if (std::isnan(x[r])) {
			++counts[edges.size() + 1];
			continue;
		}
		size_t b = 0;
		for (const PT e : edges) { b += (right ? e < x[r] : e <= x[r]) ? 1 : 0; }
		++counts[b];
	}
	return counts;
}

template <class PT>
static int run(char** argv) {
	using column = alp::gpu::column<PT>;
	const std::vector<uint8_t> blob = read_file(argv[2]), raw_edges = read_file(argv[3]), raw_mask = read_file(argv[4]);
	std::vector<PT>            edges(raw_edges.size() / sizeof(PT));
	std::memcpy(edges.data(), raw_edges.data(), edges.size() * sizeof(PT));
	std::vector<uint64_t> mask(raw_mask.size() / sizeof(uint64_t));
	std::memcpy(mask.data(), raw_mask.data(), mask.size() * sizeof(uint64_t));
	const std::vector<PT> x  = column::decompress(blob.data(), blob.size());
	const uint64_t        nv = mask.size() / 16;
	if (x.size() != nv * 1024) {
		std::printf("FAIL: %zu values, %zu mask words\n", x.size(), mask.size());
		return 1;
	}
	const std::vector<typename column::zone> masked = column::minmax_masked(blob.data(), blob.size(), mask), whole = column::zone_map(blob.data(), blob.size());
	uint64_t                                 selected = 0;
	for (const bool right : {false, true}) {
		for (const std::vector<uint64_t>* m : {static_cast<const std::vector<uint64_t>*>(nullptr), static_cast<const std::vector<uint64_t>*>(&mask)}) {
			for (const std::vector<PT>& e : {edges, std::vector<PT>(), std::vector<PT>(edges.begin(), edges.begin() + 1)}) {
				const std::vector<uint64_t> want = host_histogram(x, e, m, right);
				uint64_t                    total = 0;
				for (const uint64_t c : want) { total += c; }
				if (m) { selected = total; }
				for (const std::vector<typename column::zone>* zones : {static_cast<const std::vector<typename column::zone>*>(nullptr), &whole, &masked}) {
					if (zones == &masked && !m) { continue; } // (the masked records contain the selected values only)
					const std::vector<uint64_t> got = column::histogram(blob.data(), blob.size(), e, right, m, zones);
					if (got != want) {
						std::printf("FAIL: histogram, %zu edges, right %d, mask %d, zones %d\n", e.size(), int(right), int(m != nullptr), zones == nullptr ? 0 : zones == &whole ? 1 : 2);
						return 1;
					}
				}
			}
		}
	}
	if (selected == 0) {
		std::printf("FAIL: the mask selects nothing\n");
		return 1;
	}
	// too many edges, a mask of the wrong length and records of the wrong length throw
	int        threw = 0;
	const auto must_throw = [&](auto&& call) {
		try {
			call();
		} catch (const std::exception&) { ++threw; }
	};
	must_throw([&] { column::histogram(blob.data(), blob.size(), std::vector<PT>(ALPGPU_HISTOGRAM_EDGES_MAX + 1, PT(1))); });
	must_throw([&] {
		const std::vector<uint64_t> longer(mask.size() + 16);
		column::histogram(blob.data(), blob.size(), edges, false, &longer);
	});
	must_throw([&] {
		const std::vector<typename column::zone> few(whole.begin(), whole.end() - 1);
		column::histogram(blob.data(), blob.size(), edges, false, nullptr, &few);
	});
	if (threw != 3) {
		std::printf("FAIL: %d of 3 misuses threw\n", threw);
		return 1;
	}
	// the full 4095 edges
	std::vector<PT> many;
	for (uint32_t i = 0; i < ALPGPU_HISTOGRAM_EDGES_MAX; ++i) { many.push_back(x[(i * 7919ull) % x.size()]); }
	if (column::histogram(blob.data(), blob.size(), many, true, &mask) != host_histogram(x, many, &mask, true)) {
		std::printf("FAIL: histogram with ALPGPU_HISTOGRAM_EDGES_MAX edges\n");
		return 1;
	}
	std::printf("ok %llu %llu\n", static_cast<unsigned long long>(nv), static_cast<unsigned long long>(selected));
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 5) {
		std::printf("usage: histogram_test f64|f32 col.blob edges.bin in.mask\n");
		return 2;
	}
	try {
		return std::strcmp(argv[1], "f32") == 0 ? run<float>(argv) : run<double>(argv);
	} catch (const std::exception& e) {
		std::printf("FAIL: %s\n", e.what());
		return 1;
	}
}
