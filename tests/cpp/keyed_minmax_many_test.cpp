// keyed_minmax_many_test.cpp — alp::gpu::column<PT>::minmax_by_key_many (include/alp/batch.hpp; include/alpgpu.h, "keyed MIN / MAX, many keys") on two
// serialized columns read from files, against column::decompress and a host loop that finds a row's key by std::lower_bound and one == and orders
// values by the integer key of their bits (no float comparison: -0.0 < +0.0):
//   keyed_minmax_many_test f64|f32 val.blob key.blob keys.bin in.mask
// keys.bin holds more than ALPGPU_KEYED_KEYS_MAX keys.  Prints "ok <vectors> <selected rows> <keys>" and returns 0 when everything agrees;
// tests/test_keyed_minmax_many_gpu.py builds and runs it.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/keyed_minmax_many_test.cpp -Lalp_amd -lalpgpu -ldl
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

// the records' order: the value's bits as a signed integer, the negative half turned round
static int64_t order_key(double x) {
	int64_t b;
	std::memcpy(&b, &x, 8);
	return b >= 0 ? b : b ^ INT64_MAX;
}
static int64_t order_key(float x) {
	int32_t b;
	std::memcpy(&b, &x, 4);
	return b >= 0 ? b : b ^ INT32_MAX;
}

template <class PT>
static bool nans_last(PT a, PT b) {
	return b != b ? a == a : a < b;
}

// the definition: a selected row belongs to the first key (of the sorted list, NaNs last) equal to its key value; a row without one is unmatched; a NaN value is counted and ignored
template <class PT, class Z>
static void host_minmax_by_key(const std::vector<PT>& x, const std::vector<PT>& k, const std::vector<PT>& sorted_keys, const std::vector<uint64_t>* mask, std::vector<Z>& records,
                               std::vector<uint64_t>& counts, uint64_t& unmatched) {
	Z none;
	none.min = std::numeric_limits<PT>::infinity();
	none.max = -std::numeric_limits<PT>::infinity();
	records.assign(sorted_keys.size(), none);
	std::vector<char> has(sorted_keys.size(), 0);
	counts.assign(sorted_keys.size(), 0);
	unmatched = 0;
	size_t numbers = sorted_keys.size(); // the keys in front of the NaNs
	while (numbers > 0 && sorted_keys[numbers - 1] != sorted_keys[numbers - 1]) { --numbers; }
	for (uint64_t r = 0; r < x.size(); ++r) {
		if (mask && !(((*mask)[r >> 6] >> (r & 63)) & 1ull)) { continue; }
		const size_t i = k[r] == k[r] ? static_cast<size_t>(std::lower_bound(sorted_keys.begin(), sorted_keys.begin() + numbers, k[r]) - sorted_keys.begin()) : numbers;
		if (i >= numbers || !(sorted_keys[i] == k[r])) {
			++unmatched;
			continue;
		}
		++counts[i];
		if (x[r] != x[r]) { continue; }
		if (!has[i] || order_key(x[r]) < order_key(records[i].min)) { records[i].min = x[r]; }
		if (!has[i] || order_key(x[r]) > order_key(records[i].max)) { records[i].max = x[r]; }
		has[i] = 1;
	}
}

template <class PT>
static int run(char** argv) {
	using column = alp::gpu::column<PT>;
	using zone   = typename column::zone;
	const std::vector<uint8_t> val = read_file(argv[2]), key = read_file(argv[3]), raw_keys = read_file(argv[4]), raw_mask = read_file(argv[5]);
	std::vector<PT>            keys(raw_keys.size() / sizeof(PT));
	std::memcpy(keys.data(), raw_keys.data(), keys.size() * sizeof(PT));
	std::vector<uint64_t> mask(raw_mask.size() / sizeof(uint64_t));
	std::memcpy(mask.data(), raw_mask.data(), mask.size() * sizeof(uint64_t));
	const std::vector<PT> x = column::decompress(val.data(), val.size()), k = column::decompress(key.data(), key.size());
	const uint64_t        nv = mask.size() / 16;
	if (x.size() != nv * 1024 || k.size() != x.size()) {
		std::printf("FAIL: %zu values, %zu keys, %zu mask words\n", x.size(), k.size(), mask.size());
		return 1;
	}
	if (keys.size() <= ALPGPU_KEYED_KEYS_MAX) {
		std::printf("FAIL: %zu keys are no more than minmax_by_key takes\n", keys.size());
		return 1;
	}
	const std::vector<zone> whole = column::zone_map(key.data(), key.size());
	// the keys as given (sorted by the wrapper), reversed, with a duplicate and a NaN, the first 1024 of them, and one key alone
	std::vector<PT> reversed(keys.rbegin(), keys.rend()), extra(keys);
	extra.push_back(keys[keys.size() / 2]);
	extra.push_back(std::numeric_limits<PT>::quiet_NaN());
	const std::vector<PT> old_range(keys.begin(), keys.begin() + ALPGPU_KEYED_KEYS_MAX), one(keys.begin(), keys.begin() + 1);
	uint64_t              selected = 0;
	for (const std::vector<uint64_t>* m : {static_cast<const std::vector<uint64_t>*>(nullptr), static_cast<const std::vector<uint64_t>*>(&mask)}) {
		for (const std::vector<PT>* list : {static_cast<const std::vector<PT>*>(&keys), static_cast<const std::vector<PT>*>(&reversed), static_cast<const std::vector<PT>*>(&extra), &old_range, &one}) {
			std::vector<PT> sorted(*list);
			std::sort(sorted.begin(), sorted.end(), nans_last<PT>);
			std::vector<zone>     records;
			std::vector<uint64_t> counts;
			uint64_t              unmatched = 0;
			host_minmax_by_key(x, k, sorted, m, records, counts, unmatched);
			uint64_t total = unmatched;
			for (const uint64_t c : counts) { total += c; }
			if (m) { selected = total; }
			for (const std::vector<zone>* zones : {static_cast<const std::vector<zone>*>(nullptr), &whole}) {
				const typename column::keyed_minmax_result got = column::minmax_by_key_many(val.data(), val.size(), key.data(), key.size(), m, zones, list->data(), list->size());
				bool same = got.counts == counts && got.unmatched == unmatched && got.records.size() == records.size() && got.keys.size() == sorted.size();
				for (size_t i = 0; same && i < records.size(); ++i) {
					same = std::memcmp(&got.records[i], &records[i], sizeof(zone)) == 0 && (got.keys[i] == sorted[i] || (got.keys[i] != got.keys[i] && sorted[i] != sorted[i]));
				}
				if (!same) {
					std::printf("FAIL: minmax_by_key_many, %zu keys, mask %d, zones %d\n", list->size(), int(m != nullptr), int(zones != nullptr));
					return 1;
				}
				if (list->size() <= ALPGPU_KEYED_KEYS_MAX) { // the old range: the bytes of minmax_by_key
					const typename column::keyed_minmax_result old = column::minmax_by_key(val.data(), val.size(), key.data(), key.size(), m, zones, list->data(), list->size());
					if (old.counts != got.counts || old.unmatched != got.unmatched || std::memcmp(old.records.data(), got.records.data(), records.size() * sizeof(zone)) != 0) {
						std::printf("FAIL: minmax_by_key_many differs from minmax_by_key, %zu keys, mask %d, zones %d\n", list->size(), int(m != nullptr), int(zones != nullptr));
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
	// the column as its own key: every selected number matches the key that is its value
	size_t own_keys = 0;
	{
		std::vector<PT> own;
		for (size_t r = 0; r < x.size(); ++r) {
			if (x[r] == x[r]) { own.push_back(x[r]); }
		}
		std::sort(own.begin(), own.end());
		own.erase(std::unique(own.begin(), own.end()), own.end());
		if (own.size() > ALPGPU_KEYED_MANY_KEYS_MAX) { own.resize(ALPGPU_KEYED_MANY_KEYS_MAX); }
		own_keys = own.size();
		std::vector<zone>     records;
		std::vector<uint64_t> counts;
		uint64_t              unmatched = 0;
		host_minmax_by_key(x, x, own, &mask, records, counts, unmatched);
		const typename column::keyed_minmax_result got = column::minmax_by_key_many(val.data(), val.size(), val.data(), val.size(), &mask, nullptr, own.data(), own.size());
		if (got.counts != counts || got.unmatched != unmatched || std::memcmp(got.records.data(), records.data(), records.size() * sizeof(zone)) != 0) {
			std::printf("FAIL: minmax_by_key_many of a column by itself, %zu keys\n", own.size());
			return 1;
		}
	}
	// no keys, too many keys, a mask of the wrong length and records of the wrong length throw; minmax_by_key still stops at its own bound
	int        threw = 0;
	const auto must_throw = [&](auto&& call) {
		try {
			call();
		} catch (const std::exception&) { ++threw; }
	};
	must_throw([&] { column::minmax_by_key_many(val.data(), val.size(), key.data(), key.size(), nullptr, nullptr, keys.data(), 0); });
	must_throw([&] {
		const std::vector<PT> many(size_t(ALPGPU_KEYED_MANY_KEYS_MAX) + 1, PT(1));
		column::minmax_by_key_many(val.data(), val.size(), key.data(), key.size(), nullptr, nullptr, many.data(), many.size());
	});
	must_throw([&] {
		const std::vector<uint64_t> longer(mask.size() + 16);
		column::minmax_by_key_many(val.data(), val.size(), key.data(), key.size(), &longer, nullptr, keys.data(), keys.size());
	});
	must_throw([&] {
		const std::vector<zone> few(whole.begin(), whole.end() - 1);
		column::minmax_by_key_many(val.data(), val.size(), key.data(), key.size(), nullptr, &few, keys.data(), keys.size());
	});
	must_throw([&] { column::minmax_by_key(val.data(), val.size(), key.data(), key.size(), nullptr, nullptr, keys.data(), ALPGPU_KEYED_KEYS_MAX + 1); });
	if (threw != 5) {
		std::printf("FAIL: %d of 5 misuses threw\n", threw);
		return 1;
	}
	std::printf("ok %llu %llu %zu %zu\n", static_cast<unsigned long long>(nv), static_cast<unsigned long long>(selected), keys.size(), own_keys);
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 6) {
		std::printf("usage: keyed_minmax_many_test f64|f32 val.blob key.blob keys.bin in.mask\n");
		return 2;
	}
	try {
		if (std::strcmp(argv[1], "f64") == 0) { return run<double>(argv); }
		if (std::strcmp(argv[1], "f32") == 0) { return run<float>(argv); }
		throw std::runtime_error("the first argument is f64 or f32");
	} catch (const std::exception& e) {
		std::printf("FAIL: %s\n", e.what());
		return 1;
	}
}
