// distinct_test.cpp — alp::gpu::column<PT>::distinct (include/alp/batch.hpp; include/alpgpu.h, "distinct values") on a serialized column read from a
// file, against column::decompress and a host loop over the definition (an ordered map by <, the zeros one key, NaNs counted apart):
//   distinct_test f64|f32 col.blob in.mask
// Prints "ok <vectors> <distinct values under the mask>" and returns 0 when everything agrees; tests/test_distinct_gpu.py builds and runs it.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/distinct_test.cpp -Lalp_amd -lalpgpu -ldl
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
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
struct host_result {
	std::vector<PT>       values;
	std::vector<uint64_t> counts;
	uint64_t              nans = 0, numbers = 0;
};

// the definition: equality is ==, so the two zeros share a key (std::map's < finds neither below the other), reported as +0.0
template <class PT>
static host_result<PT> host_distinct(const std::vector<PT>& x, const std::vector<uint64_t>* mask) {
	std::map<PT, uint64_t> seen;
	host_result<PT>        out;
	for (uint64_t r = 0; r < x.size(); ++r) {
		if (mask && !(((*mask)[r >> 6] >> (r & 63)) & 1ull)) { continue; }
		if (std::isnan(x[r])) {
			++out.nans;
			continue;
		}
		++out.numbers;
		++seen[x[r] == PT(0) ? PT(0) : x[r]];
	}
	for (const auto& kv : seen) {
		out.values.push_back(kv.first);
		out.counts.push_back(kv.second);
	}
	return out;
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
	const std::vector<typename column::zone> masked = column::minmax_masked(blob.data(), blob.size(), mask), whole = column::zone_map(blob.data(), blob.size());
	uint64_t                                 under_mask = 0;
	for (const std::vector<uint64_t>* m : {static_cast<const std::vector<uint64_t>*>(nullptr), static_cast<const std::vector<uint64_t>*>(&mask)}) {
		const host_result<PT> want = host_distinct(x, m);
		if (m) { under_mask = want.values.size(); }
		for (const std::vector<typename column::zone>* zones : {static_cast<const std::vector<typename column::zone>*>(nullptr), &whole, &masked}) {
			if (zones == &masked && !m) { continue; } // (the masked records contain the selected values only)
			for (const uint64_t capacity : {uint64_t(65536), uint64_t(want.values.size() > 0 ? want.values.size() : 1)}) {
				const typename column::distinct_result got = column::distinct(blob.data(), blob.size(), m, zones, capacity);
				const bool same = !got.overflow && got.nans == want.nans && got.numbers == want.numbers && got.counts == want.counts && got.values.size() == want.values.size() &&
				                  (got.values.empty() || std::memcmp(got.values.data(), want.values.data(), got.values.size() * sizeof(PT)) == 0);
				if (!same) {
					std::printf("FAIL: distinct, mask %d, zones %d, capacity %llu: %zu values (want %zu), overflow %d\n", int(m != nullptr), zones == nullptr ? 0 : zones == &whole ? 1 : 2,
					            static_cast<unsigned long long>(capacity), got.values.size(), want.values.size(), int(got.overflow));
					return 1;
				}
			}
		}
		// one entry too few: the overflow flag, the two totals still right, nothing returned
		if (want.values.size() > 1) {
			const typename column::distinct_result got = column::distinct(blob.data(), blob.size(), m, nullptr, want.values.size() - 1);
			if (!got.overflow || got.nans != want.nans || got.numbers != want.numbers || !got.values.empty() || !got.counts.empty()) {
				std::printf("FAIL: distinct with one entry too few, mask %d\n", int(m != nullptr));
				return 1;
			}
		}
		// the values are the point buckets' edges: bucket i + 1 of the histogram counts value i
		if (want.values.size() > ALPGPU_HISTOGRAM_EDGES_MAX) {
			std::printf("FAIL: the column has more distinct values than a histogram takes edges\n");
			return 1;
		}
		const typename column::distinct_result again = column::distinct(blob.data(), blob.size(), m);
		const std::vector<uint64_t>            hist  = column::histogram(blob.data(), blob.size(), again.values, false, m);
		for (size_t i = 0; i < again.values.size(); ++i) {
			if (hist[i + 1] != again.counts[i]) {
				std::printf("FAIL: histogram by the distinct values, bucket %zu\n", i + 1);
				return 1;
			}
		}
	}
	if (under_mask == 0) {
		std::printf("FAIL: the mask selects no number\n");
		return 1;
	}
	// a capacity outside 1 .. ALPGPU_DISTINCT_MAX, a mask of the wrong length and records of the wrong length throw
	int        threw = 0;
	const auto must_throw = [&](auto&& call) {
		try {
			call();
		} catch (const std::exception&) { ++threw; }
	};
	must_throw([&] { column::distinct(blob.data(), blob.size(), nullptr, nullptr, 0); });
	must_throw([&] { column::distinct(blob.data(), blob.size(), nullptr, nullptr, uint64_t(ALPGPU_DISTINCT_MAX) + 1); });
	must_throw([&] {
		const std::vector<uint64_t> longer(mask.size() + 16);
		column::distinct(blob.data(), blob.size(), &longer);
	});
	must_throw([&] {
		const std::vector<typename column::zone> few(whole.begin(), whole.end() - 1);
		column::distinct(blob.data(), blob.size(), nullptr, &few);
	});
	if (threw != 4) {
		std::printf("FAIL: %d of 4 misuses threw\n", threw);
		return 1;
	}
	std::printf("ok %llu %llu\n", static_cast<unsigned long long>(nv), static_cast<unsigned long long>(under_mask));
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 4) {
		std::printf("usage: distinct_test f64|f32 col.blob in.mask\n");
		return 2;
	}
	try {
		return std::strcmp(argv[1], "f32") == 0 ? run<float>(argv) : run<double>(argv);
	} catch (const std::exception& e) {
		std::printf("FAIL: %s\n", e.what());
		return 1;
	}
}
