// exact_sum_host.cpp — alp_amd/csrc/exact_sum.hpp alone on the host (no HIP, no library): the split of a double into its limb and chunks, the limbs'
// accumulation and exact_round_limbs.  tests/test_keyed_sum_exact_cpu.py builds it with -fsanitize=address,undefined, feeds it lists and compares what
// it prints with tests/keyed_exact_replica.py (Python integers).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ialp_amd/csrc tests/cpp/exact_sum_host.cpp
// stdin, one case per line:
//   v <hex bits of a double> ...             the values of one key; prints the bits of their exactly rounded sum
//   l <flags> <66 limbs, decimal int64>      a table entry as it is; prints the bits of exact_round_limbs
// stdout: one line of 16 hex digits per case.
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "exact_sum.hpp"

int main() {
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string        kind;
		if (!(in >> kind)) { continue; }
		int64_t  limbs[alpgpu::kExactLimbs] = {};
		uint64_t flags                      = 0;
		if (kind == "v") {
			std::string word;
			while (in >> word) {
				const uint64_t bits = std::stoull(word, nullptr, 16);
				double         x;
				memcpy(&x, &bits, sizeof x);
				alpgpu::exact_add(limbs, flags, x);
			}
		} else if (kind == "l") {
			in >> flags;
			for (uint32_t j = 0; j < alpgpu::kExactLimbs; ++j) {
				if (!(in >> limbs[j])) {
					std::fprintf(stderr, "a table entry has 66 limbs\n");
					return 2;
				}
			}
		} else {
			std::fprintf(stderr, "unknown case '%s'\n", kind.c_str());
			return 2;
		}
		const double   r = alpgpu::exact_round_limbs(limbs, flags);
		uint64_t       b;
		memcpy(&b, &r, sizeof b);
		std::printf("%016" PRIx64 "\n", b);
	}
	return 0;
}
