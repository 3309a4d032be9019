// persistent_launch_test.cpp — the launch rules of the persistent scan kernels (alp_amd/csrc/persistent_launch.hpp) evaluated on the host, without a GPU,
// HIP or the library:
//   g++ -std=c++17 -I alp_amd/csrc tests/cpp/persistent_launch_test.cpp
// Reads rows from stdin and prints one line per row:
//   G vectors waves n_cus wg_per_cu resident_cap grid_override override_max   ->  grid
//   S n_list value_bytes                                                      ->  stride n_piv lds_max
// tests/test_persistent_launch_cpu.py compares.
#include <cinttypes>
#include <cstdio>

#include "persistent_launch.hpp"

int main() {
	char line[256];
	while (fgets(line, sizeof line, stdin)) {
		uint64_t vectors, cap, n_list;
		uint32_t waves, wg_per_cu, grid_override, override_max;
		int      n_cus, value_bytes;
		if (sscanf(line, "G %" SCNu64 " %" SCNu32 " %d %" SCNu32 " %" SCNu64 " %" SCNu32 " %" SCNu32, &vectors, &waves, &n_cus, &wg_per_cu, &cap, &grid_override, &override_max) == 7) {
			printf("%u\n", alpgpu::persistent_grid(vectors, waves, n_cus, wg_per_cu, cap, grid_override, override_max));
		} else if (sscanf(line, "S %" SCNu64 " %d", &n_list, &value_bytes) == 2) {
			const alpgpu::ListStaging s = alpgpu::list_staging(n_list, value_bytes);
			printf("%u %u %zu\n", s.stride, s.n_piv, alpgpu::in_list_lds_max(value_bytes));
		} else {
			fprintf(stderr, "bad row: %s", line);
			return 1;
		}
	}
	return 0;
}
