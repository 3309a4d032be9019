// keyed_sum_exact_test.cpp — alp::gpu::column<PT>::sum_by_key_exact (include/alp/batch.hpp; include/alpgpu.h, "exact keyed SUM") on two serialized
// columns read from files.  The counts are held to column::decompress and a host loop that finds a row's key by std::lower_bound and one ==; the
// sums, byte for byte, to want.bin, which tests/test_keyed_sum_exact_gpu.py wrote from its host replica (Python integers) for the sorted keys under
// the mask: K doubles, then K + 1 counts.
//   keyed_sum_exact_test f64|f32 val.blob key.blob keys.bin in.mask want.bin
// keys.bin holds more than ALPGPU_KEYED_KEYS_MAX keys, in any order.  Prints "ok <vectors> <selected rows> <keys>" and returns 0 when everything agrees.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/keyed_sum_exact_test.cpp -Lalp_amd -lalpgpu -ldl
#include <algorithm>
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

template <class PT>
static bool nans_last(PT a, PT b) {
	return b != b ? a == a : a < b;
}

// the definition of the counts: a selected row belongs to the first key (of the sorted list, NaNs last) equal to its key value; a row without one is unmatched
template <class PT>
static void host_count_by_key(const std::vector<PT>& k, const std::vector<PT>& sorted_keys, const std::vector<uint64_t>* mask, std::vector<uint64_t>& counts, uint64_t& unmatched) {
	counts.assign(sorted_keys.size(), 0);
	unmatched      = 0;
	size_t numbers = sorted_keys.size(); // the keys in front of the NaNs
	while (numbers > 0 && sorted_keys[numbers - 1] != sorted_keys[numbers - 1]) { --numbers; }
	for (uint64_t r = 0; r < k.size(); ++r) {
		if (mask && !(((*mask)[r >> 6] >> (r & 63)) & 1ull)) { continue; }
		const size_t i = k[r] == k[r] ? static_cast<size_t>(std::lower_bound(sorted_keys.begin(), sorted_keys.begin() + numbers, k[r]) - sorted_keys.begin()) : numbers;
		if (i >= numbers || !(sorted_keys[i] == k[r])) {
			++unmatched;
		} else {
			++counts[i];
		}
	}
}

template <class PT>
static int run(char** argv) {
	using column = alp::gpu::column<PT>;
	using zone   = typename column::zone;
	const std::vector<uint8_t> val = read_file(argv[2]), key = read_file(argv[3]), raw_keys = read_file(argv[4]), raw_mask = read_file(argv[5]), raw_want = read_file(argv[6]);
	std::vector<PT>            keys(raw_keys.size() / sizeof(PT));
	std::memcpy(keys.data(), raw_keys.data(), keys.size() * sizeof(PT));
	std::vector<uint64_t> mask(raw_mask.size() / sizeof(uint64_t));
	std::memcpy(mask.data(), raw_mask.data(), mask.size() * sizeof(uint64_t));
	const size_t K = keys.size();
	if (K <= ALPGPU_KEYED_KEYS_MAX || raw_want.size() != 8 * K + 8 * (K + 1)) {
		std::printf("FAIL: %zu keys (more than sum_by_key takes are expected), %zu bytes of expectation\n", K, raw_want.size());
		return 1;
	}
	std::vector<double>   want_sums(K);
	std::vector<uint64_t> want_counts(K + 1);
	std::memcpy(want_sums.data(), raw_want.data(), 8 * K);
	std::memcpy(want_counts.data(), raw_want.data() + 8 * K, 8 * (K + 1));
	const std::vector<PT> k  = column::decompress(key.data(), key.size());
	const uint64_t        nv = mask.size() / 16;
	if (k.size() != nv * 1024) {
		std::printf("FAIL: %zu keys, %zu mask words\n", k.size(), mask.size());
		return 1;
	}
	std::vector<PT> sorted(keys);
	std::sort(sorted.begin(), sorted.end(), nans_last<PT>);
	std::vector<uint64_t> counts;
	uint64_t              unmatched = 0, selected = 0;
	host_count_by_key(k, sorted, &mask, counts, unmatched);
	for (const uint64_t c : counts) { selected += c; }
	selected += unmatched;
	if (!std::equal(counts.begin(), counts.end(), want_counts.begin()) || unmatched != want_counts[K]) {
		std::printf("FAIL: the expectation's counts are not the host loop's\n");
		return 1;
	}
	const std::vector<zone> whole = column::zone_map(key.data(), key.size());
	const std::vector<PT>   reversed(keys.rbegin(), keys.rend());
	for (const std::vector<PT>* list : {static_cast<const std::vector<PT>*>(&keys), &reversed}) {
		for (const std::vector<zone>* zones : {static_cast<const std::vector<zone>*>(nullptr), &whole}) {
			const typename column::keyed_result got = column::sum_by_key_exact(val.data(), val.size(), key.data(), key.size(), &mask, zones, list->data(), list->size());
			if (got.keys.size() != K || got.sums.size() != K || got.counts != counts || got.unmatched != unmatched || std::memcmp(got.keys.data(), sorted.data(), K * sizeof(PT)) != 0 ||
			    std::memcmp(got.sums.data(), want_sums.data(), 8 * K) != 0) {
				std::printf("FAIL: sum_by_key_exact, %zu keys, zones %d\n", K, int(zones != nullptr));
				return 1;
			}
		}
	}
	// without a mask: the counts are the host loop's over every row, and the sums do not depend on the zone map
	{
		host_count_by_key(k, sorted, nullptr, counts, unmatched);
		const typename column::keyed_result a = column::sum_by_key_exact(val.data(), val.size(), key.data(), key.size(), nullptr, nullptr, keys.data(), K);
		const typename column::keyed_result b = column::sum_by_key_exact(val.data(), val.size(), key.data(), key.size(), nullptr, &whole, keys.data(), K);
		if (a.counts != counts || a.unmatched != unmatched || b.counts != counts || std::memcmp(a.sums.data(), b.sums.data(), 8 * K) != 0) {
			std::printf("FAIL: sum_by_key_exact without a mask\n");
			return 1;
		}
	}
	// no keys, too many keys, a mask of the wrong length and records of the wrong length throw
	int        threw      = 0;
	const auto must_throw = [&](auto&& call) {
		try {
			call();
		} catch (const std::exception&) { ++threw; }
	};
	must_throw([&] { column::sum_by_key_exact(val.data(), val.size(), key.data(), key.size(), nullptr, nullptr, keys.data(), 0); });
	must_throw([&] {
		const std::vector<PT> many(size_t(ALPGPU_KEYED_MANY_KEYS_MAX) + 1, PT(1));
		column::sum_by_key_exact(val.data(), val.size(), key.data(), key.size(), nullptr, nullptr, many.data(), many.size());
	});
	must_throw([&] {
		const std::vector<uint64_t> longer(mask.size() + 16);
		column::sum_by_key_exact(val.data(), val.size(), key.data(), key.size(), &longer, nullptr, keys.data(), K);
	});
	must_throw([&] {
		const std::vector<zone> few(whole.begin(), whole.end() - 1);
		column::sum_by_key_exact(val.data(), val.size(), key.data(), key.size(), nullptr, &few, keys.data(), K);
	});
	if (threw != 4) {
		std::printf("FAIL: %d of 4 misuses threw\n", threw);
		return 1;
	}
	std::printf("ok %llu %llu %zu\n", static_cast<unsigned long long>(nv), static_cast<unsigned long long>(selected), K);
	return 0;
}

int main(int argc, char** argv) {
	if (argc != 7) {
		std::printf("usage: keyed_sum_exact_test f64|f32 val.blob key.blob keys.bin in.mask want.bin\n");
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
