// rd_order_test.cpp — the device's replay of libstdc++'s containers (alp_amd/csrc/rd_dictionary_order.hpp) held against the containers
// themselves, on the host, without a GPU or the library:
//   g++ -std=c++17 -I alp_amd/csrc tests/cpp/rd_order_test.cpp            (and once more with -fsanitize=address,undefined)
// Reads one case per line from stdin, "D key_0 count_0 ... key_{D-1} count_{D-1}": the D distinct left parts of a sample in order of first
// occurrence with their counts (what k_rowgroup_init hands rd_reference_order).  Prints two lines per case: "replay ..." = the keys in
// the order rd_reference_order leaves them, "std ..." = the keys as std::unordered_map<uint64_t, int32_t> + std::sort by count leave them
// (include/alp/rd.hpp:33-54 of the reference does exactly that with these containers).  The last line is "heap_sorts N": how often the
// replay's introsort ran out of depth and fell back to heap sort.  tests/test_rd_search_cpu.py compares.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <unordered_map>
#include <utility>
#include <vector>

static long g_heap_sorts = 0;
#define ALPGPU_RD_ORDER_ON_HEAP_SORT (++g_heap_sorts)
#include "rd_dictionary_order.hpp"

static std::vector<uint64_t> std_order(const std::vector<std::pair<uint64_t, int32_t>>& first_occurrence) {
	std::unordered_map<uint64_t, int32_t> hash;
	for (auto& kc : first_occurrence) { hash[kc.first] += kc.second; } // (a key enters the map at its first occurrence; later ones only count)
	std::vector<std::pair<int, uint64_t>> sorted;
	sorted.reserve(hash.size());
	for (auto& pair : hash) { sorted.emplace_back(pair.second, pair.first); }
	std::sort(sorted.begin(), sorted.end(), [](const std::pair<int, uint64_t>& a, const std::pair<int, uint64_t>& b) { return a.first > b.first; });
	std::vector<uint64_t> keys;
	for (auto& p : sorted) { keys.push_back(p.second); }
	return keys;
}

int main() {
	static alpgpu::RdOrderLds X;
	int                       D;
	while (scanf("%d", &D) == 1) {
		if (D < 0 || D > alpgpu::kRdMaxDistinct) {
			fprintf(stderr, "D = %d is outside 0..%d\n", D, alpgpu::kRdMaxDistinct);
			return 1;
		}
		std::vector<std::pair<uint64_t, int32_t>> in;
		for (int i = 0; i < D; ++i) {
			unsigned key, count;
			if (scanf("%u %u", &key, &count) != 2 || key > 0xFFFFu || count == 0 || count > 0xFFFFu) {
				fprintf(stderr, "bad (key, count) pair\n");
				return 1;
			}
			in.emplace_back(key, static_cast<int32_t>(count));
			X.okey[i] = key;
			X.ocnt[i] = count;
		}
		alpgpu::rd_reference_order(X, D);
		printf("replay");
		for (int i = 0; i < D; ++i) { printf(" %u", X.sorted[i] & 0xFFFFu); }
		printf("\nstd");
		for (uint64_t k : std_order(in)) { printf(" %u", static_cast<unsigned>(k)); }
		printf("\n");
	}
	printf("heap_sorts %ld\n", g_heap_sorts);
	return 0;
}
