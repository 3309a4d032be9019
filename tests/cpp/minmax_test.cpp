// minmax_test.cpp — alp::gpu::column<PT>::minmax_masked / group_minmax_masked / group_minmax_totals (include/alp/batch.hpp; include/alpgpu.h,
// "masked and grouped MIN / MAX") on two serialized columns read from files, against column::decompress and a host loop over the definition of a
// record, bit for bit:
//   minmax_test f64|f32 val.blob key.blob in.mask bounds.bin
// bounds.bin holds n_groups lower bounds and then n_groups upper bounds in the columns' type.  Prints "ok <vectors> <groups> <records that are not
// empty>" and returns 0 when everything agrees; tests/test_minmax_gpu.py builds and runs it.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/minmax_test.cpp -Lalp_amd -lalpgpu -ldl
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <limits>
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

// the order-preserving key of a value's bits: ascending keys = ascending values, -0.0 below +0.0
template <class PT>
static int64_t order_key(PT x) {
	typename std::conditional<sizeof(PT) == 8, int64_t, int32_t>::type b;
	std::memcpy(&b, &x, sizeof(b));
	return b >= 0 ? b : b ^ std::numeric_limits<decltype(b)>::max();
}

// the record of the values taken so far, by the definition: NaNs ignored, {+inf, -inf} for none
template <class PT>
struct host_record {
	PT   min = std::numeric_limits<PT>::infinity(), max = -std::numeric_limits<PT>::infinity();
	bool any = false;
	void take(PT x) {
		if (std::isnan(x)) { return; }
		if (!any || order_key(x) < order_key(min)) { min = x; }
		if (!any || order_key(x) > order_key(max)) { max = x; }
		any = true;
	}
	template <class Z>
	bool same(const Z& z) const { return std::memcmp(&z.min, &min, sizeof(PT)) == 0 && std::memcmp(&z.max, &max, sizeof(PT)) == 0; }
};

template <class PT>
static int run(char** argv) {
	using column = alp::gpu::column<PT>;
	using zone   = typename column::zone;
	const std::vector<uint8_t> val = read_file(argv[2]), key = read_file(argv[3]), raw_mask = read_file(argv[4]), raw_bounds = read_file(argv[5]);
	std::vector<uint64_t>      mask(raw_mask.size() / sizeof(uint64_t));
	std::memcpy(mask.data(), raw_mask.data(), mask.size() * sizeof(uint64_t));
	std::vector<PT> bounds(raw_bounds.size() / sizeof(PT));
	std::memcpy(bounds.data(), raw_bounds.data(), bounds.size() * sizeof(PT));
	const uint32_t        n_groups = static_cast<uint32_t>(bounds.size() / 2);
	const PT *            lo = bounds.data(), *hi = bounds.data() + n_groups;
	const std::vector<PT> x = column::decompress(val.data(), val.size()), k = column::decompress(key.data(), key.size());
	const auto            bit = [&](uint64_t r) { return (mask[r >> 6] >> (r & 63)) & 1ull; };

	// the masked records and their counts
	std::vector<uint32_t>   counts;
	const std::vector<zone> zones = column::minmax_masked(val.data(), val.size(), mask, &counts);
	const uint64_t          nv    = zones.size();
	if (mask.size() != 16 * nv || x.size() != nv * 1024 || k.size() != x.size() || counts.size() != nv) {
		std::printf("FAIL: %zu records, %zu counts, %zu and %zu values, %zu mask words\n", zones.size(), counts.size(), x.size(), k.size(), mask.size());
		return 1;
	}
	uint64_t not_empty = 0;
	for (uint64_t v = 0; v < nv; ++v) {
		host_record<PT> want;
		uint32_t        n = 0;
		for (uint64_t r = 1024 * v; r < 1024 * (v + 1); ++r) {
			if (bit(r)) {
				want.take(x[r]);
				++n;
			}
		}
		if (!want.same(zones[v]) || counts[v] != n) {
			std::printf("FAIL: minmax_masked, vector %llu\n", static_cast<unsigned long long>(v));
			return 1;
		}
		not_empty += want.any;
	}
	const std::vector<zone> again = column::minmax_masked(val.data(), val.size(), mask);
	if (std::memcmp(again.data(), zones.data(), nv * sizeof(zone)) != 0) {
		std::printf("FAIL: the records without counts differ\n");
		return 1;
	}

	// the grouped records, their counts and every group's total
	std::vector<zone>     gz;
	std::vector<uint32_t> gc;
	if (column::group_minmax_masked(val.data(), val.size(), key.data(), key.size(), mask, lo, hi, n_groups, gz, &gc) != nv || gz.size() != n_groups * nv || gc.size() != gz.size()) {
		std::printf("FAIL: group_minmax_masked's shapes\n");
		return 1;
	}
	const std::vector<zone> totals = column::group_minmax_totals(gz, nv, n_groups);
	for (uint32_t g = 0; g < n_groups; ++g) {
		host_record<PT> total;
		for (uint64_t v = 0; v < nv; ++v) {
			host_record<PT> want;
			uint32_t        n = 0;
			for (uint64_t r = 1024 * v; r < 1024 * (v + 1); ++r) {
				if (bit(r) && k[r] >= lo[g] && k[r] <= hi[g]) {
					want.take(x[r]);
					total.take(x[r]);
					++n;
				}
			}
			if (!want.same(gz[g * nv + v]) || gc[g * nv + v] != n) {
				std::printf("FAIL: group_minmax_masked, group %u vector %llu\n", g, static_cast<unsigned long long>(v));
				return 1;
			}
			not_empty += want.any;
		}
		if (!total.same(totals[g])) {
			std::printf("FAIL: group_minmax_totals, group %u\n", g);
			return 1;
		}
	}
	const std::vector<zone> none = column::group_minmax_totals(std::vector<zone>(), 0, 2);
	if (none.size() != 2 || !host_record<PT>().same(none[0]) || !host_record<PT>().same(none[1])) {
		std::printf("FAIL: group_minmax_totals of no vectors\n");
		return 1;
	}

	// a mask of the wrong length, no group, too many groups, and records of the wrong shape, throw
	int threw = 0;
	try {
		column::minmax_masked(val.data(), val.size(), std::vector<uint64_t>(mask.size() + 16));
	} catch (const std::exception&) { ++threw; }
	try {
		column::group_minmax_masked(val.data(), val.size(), key.data(), key.size(), std::vector<uint64_t>(mask.size() + 16), lo, hi, n_groups, gz);
	} catch (const std::exception&) { ++threw; }
	try {
		column::group_minmax_masked(val.data(), val.size(), key.data(), key.size(), mask, lo, hi, 0, gz);
	} catch (const std::exception&) { ++threw; }
	try {
		const std::vector<PT> many(ALPGPU_GROUP_MAX + 1, PT(0));
		column::group_minmax_masked(val.data(), val.size(), key.data(), key.size(), mask, many.data(), many.data(), ALPGPU_GROUP_MAX + 1, gz);
	} catch (const std::exception&) { ++threw; }
	try {
		column::group_minmax_totals(totals, nv + 1, n_groups);
	} catch (const std::exception&) { ++threw; }
	if (threw != 5) {
		std::printf("FAIL: %d of 5 misuses threw\n", threw);
		return 1;
	}
	std::printf("ok %llu %u %llu\n", static_cast<unsigned long long>(nv), n_groups, static_cast<unsigned long long>(not_empty));
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 6) {
		std::printf("usage: minmax_test f64|f32 val.blob key.blob in.mask bounds.bin\n");
		return 2;
	}
	try {
		return std::strcmp(argv[1], "f32") == 0 ? run<float>(argv) : run<double>(argv);
	} catch (const std::exception& e) {
		std::printf("FAIL: %s\n", e.what());
		return 1;
	}
}
