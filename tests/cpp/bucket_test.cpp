// bucket_test.cpp — alp::gpu::column<PT>::sum_by_bucket and ::minmax_by_bucket (include/alp/batch.hpp; include/alpgpu.h, "bucketed aggregation") on two
// serialized columns read from files, against column::decompress and a host loop.  The value column holds whole numbers of at most 21 bits, so every
// partial sum is exact and no order of addition changes a bit:
//   bucket_test f64|f32 val.blob key.blob edges.bin in.mask
// Prints "ok <vectors> <selected rows>" and returns 0 when everything agrees; tests/test_bucket_gpu.py builds and runs it.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/bucket_test.cpp -Lalp_amd -lalpgpu -ldl
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <limits>
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

// the definition: a selected row whose key is no NaN lies in bucket b = #{e <= k} (right: #{e < k}); NaN edges are inert
template <class PT>
static void host_by_bucket(const std::vector<PT>& x, const std::vector<PT>& k, const std::vector<PT>& edges, bool right, const std::vector<uint64_t>* mask, std::vector<double>& sums,
                           std::vector<PT>& mins, std::vector<PT>& maxs, std::vector<uint64_t>& counts, uint64_t& nan_keys) {
	const PT inf = std::numeric_limits<PT>::infinity();
	sums.assign(edges.size() + 1, 0.0);
	mins.assign(edges.size() + 1, inf);
	maxs.assign(edges.size() + 1, -inf);
	counts.assign(edges.size() + 1, 0);
	nan_keys = 0;
	for (uint64_t r = 0; r < x.size(); ++r) {
		if (mask && !(((*mask)[r >> 6] >> (r & 63)) & 1ull)) { continue; }
		if (k[r] != k[r]) {
			++nan_keys;
			continue;
		}
		size_t b = 0;
		for (const PT e : edges) { b += (right ? e < k[r] : e <= k[r]) ? 1 : 0; }
		sums[b] += static_cast<double>(x[r]);
		mins[b] = std::min(mins[b], x[r]); // (whole numbers, no -0.0 and no NaN: C's order is the records')
		maxs[b] = std::max(maxs[b], x[r]);
		++counts[b];
	}
}

template <class PT>
static int run(char** argv) {
	using column = alp::gpu::column<PT>;
	const std::vector<uint8_t> val = read_file(argv[2]), key = read_file(argv[3]), raw_edges = read_file(argv[4]), raw_mask = read_file(argv[5]);
	std::vector<PT>            edges(raw_edges.size() / sizeof(PT));
	std::memcpy(edges.data(), raw_edges.data(), edges.size() * sizeof(PT));
	std::vector<uint64_t> mask(raw_mask.size() / sizeof(uint64_t));
	std::memcpy(mask.data(), raw_mask.data(), mask.size() * sizeof(uint64_t));
	const std::vector<PT> x = column::decompress(val.data(), val.size()), k = column::decompress(key.data(), key.size());
	const uint64_t        nv = mask.size() / 16;
	if (x.size() != nv * 1024 || k.size() != x.size()) {
		std::printf("FAIL: %zu values, %zu keys, %zu mask words\n", x.size(), k.size(), mask.size());
		return 1;
	}
	for (const PT v : x) {
		if (!(std::fabs(static_cast<double>(v)) <= 1048576.0) || std::floor(static_cast<double>(v)) != static_cast<double>(v) || (v == 0 && std::signbit(v))) {
			std::printf("FAIL: the value column must hold whole numbers of at most 21 bits and no -0.0\n");
			return 1;
		}
	}
	const std::vector<typename column::zone> whole = column::zone_map(key.data(), key.size());
	// the edges as given (sorted by the wrapper), reversed, with a duplicate and a NaN, one edge alone and none
	std::vector<PT> reversed(edges.rbegin(), edges.rend()), extra(edges);
	extra.push_back(edges[edges.size() / 2]);
	extra.push_back(std::nan(""));
	const std::vector<PT> one(edges.begin(), edges.begin() + 1), none;
	uint64_t              selected = 0;
	for (const std::vector<uint64_t>* m : {static_cast<const std::vector<uint64_t>*>(nullptr), static_cast<const std::vector<uint64_t>*>(&mask)}) {
		for (const std::vector<PT>* list : {static_cast<const std::vector<PT>*>(&edges), static_cast<const std::vector<PT>*>(&reversed), static_cast<const std::vector<PT>*>(&extra), &one, &none}) {
			for (const bool right : {false, true}) {
				std::vector<PT> sorted(*list);
				std::sort(sorted.begin(), sorted.end(), [](PT a, PT b) { return b != b ? a == a : a < b; });
				std::vector<double>   sums;
				std::vector<PT>       mins, maxs;
				std::vector<uint64_t> counts;
				uint64_t              nan_keys = 0;
				host_by_bucket(x, k, sorted, right, m, sums, mins, maxs, counts, nan_keys);
				uint64_t total = nan_keys;
				for (const uint64_t c : counts) { total += c; }
				if (m) { selected = total; }
				for (const std::vector<typename column::zone>* zones : {static_cast<const std::vector<typename column::zone>*>(nullptr), &whole}) {
					const typename column::bucket_result s = column::sum_by_bucket(val.data(), val.size(), key.data(), key.size(), m, zones, list->data(), list->size(), right);
					const typename column::bucket_result r = column::minmax_by_bucket(val.data(), val.size(), key.data(), key.size(), m, zones, list->data(), list->size(), right);
					bool same = s.counts == counts && r.counts == counts && s.nan_keys == nan_keys && r.nan_keys == nan_keys && s.sums.size() == sums.size() &&
					            r.records.size() == sums.size() && s.edges.size() == sorted.size() && s.records.empty() && r.sums.empty();
					for (size_t i = 0; same && i < sums.size(); ++i) {
						same = std::memcmp(&s.sums[i], &sums[i], sizeof(double)) == 0 && std::memcmp(&r.records[i].min, &mins[i], sizeof(PT)) == 0 &&
						       std::memcmp(&r.records[i].max, &maxs[i], sizeof(PT)) == 0;
					}
					for (size_t i = 0; same && i < sorted.size(); ++i) { same = s.edges[i] == sorted[i] || (s.edges[i] != s.edges[i] && sorted[i] != sorted[i]); }
					if (!same) {
						std::printf("FAIL: by bucket, %zu edges, right %d, mask %d, zones %d\n", list->size(), int(right), int(m != nullptr), int(zones != nullptr));
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
	// too many edges, NULL edges with a count, a mask of the wrong length and records of the wrong length throw
	int        threw = 0;
	const auto must_throw = [&](auto&& call) {
		try {
			call();
		} catch (const std::exception&) { ++threw; }
	};
	must_throw([&] {
		const std::vector<PT> many(ALPGPU_BUCKET_EDGES_MAX + 1, PT(1));
		column::sum_by_bucket(val.data(), val.size(), key.data(), key.size(), nullptr, nullptr, many.data(), many.size());
	});
	must_throw([&] { column::minmax_by_bucket(val.data(), val.size(), key.data(), key.size(), nullptr, nullptr, nullptr, 3); });
	must_throw([&] {
		const std::vector<uint64_t> longer(mask.size() + 16);
		column::sum_by_bucket(val.data(), val.size(), key.data(), key.size(), &longer, nullptr, edges.data(), edges.size());
	});
	must_throw([&] {
		const std::vector<typename column::zone> few(whole.begin(), whole.end() - 1);
		column::minmax_by_bucket(val.data(), val.size(), key.data(), key.size(), nullptr, &few, edges.data(), edges.size());
	});
	if (threw != 4) {
		std::printf("FAIL: %d of 4 misuses threw\n", threw);
		return 1;
	}
	std::printf("ok %llu %llu\n", static_cast<unsigned long long>(nv), static_cast<unsigned long long>(selected));
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 6) {
		std::printf("usage: bucket_test f64|f32 val.blob key.blob edges.bin in.mask\n");
		return 2;
	}
	try {
		if (std::strcmp(argv[1], "f64") == 0) { return run<double>(argv); }
		if (std::strcmp(argv[1], "f32") == 0) { return run<float>(argv); }
		throw std::runtime_error("the type must be f64 or f32");
	} catch (const std::exception& e) {
		std::printf("FAIL: %s\n", e.what());
		return 1;
	}
}
