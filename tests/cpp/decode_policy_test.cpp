// decode_policy_test.cpp — the store decode's launch rule (alp_amd/csrc/decode_policy.hpp) evaluated on the host, without a GPU or the library:
//   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I alp_amd/csrc tests/cpp/decode_policy_test.cpp
// Reads rows "value_bytes n_vectors packed_bytes exc_bytes rd_rowgroups_hint exceptions rd_vectors forced_vpw forced_pad read_ahead streams_serialize plain_stores
// lead_us" from stdin (anything behind a '|' is ignored, '#' lines are skipped) and prints per row what tests/golden/decode_plan_sweep.txt records:
//   debug_word vectors_per_wg reads_ahead stretch_kind unhinted_shape unhinted_ahead lead_min lead_max ps_per_vector
// tests/test_decode_policy_cpu.py compares.
#include <cinttypes>
#include <cstdio>

#include "decode_policy.hpp"

int main() {
	char line[512];
	while (fgets(line, sizeof line, stdin)) {
		if (line[0] == '#' || line[0] == '\n') { continue; }
		int      vb, vpw, pad, ra, ser, plain, lead_us;
		uint64_t n, packed, exc, rd_hint, exceptions, rd_vectors;
		if (sscanf(line, "%d %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %d %d %d %d %d %d", &vb, &n, &packed, &exc, &rd_hint, &exceptions, &rd_vectors, &vpw,
		           &pad, &ra, &ser, &plain, &lead_us) != 13) {
			fprintf(stderr, "bad row: %s", line);
			return 1;
		}
		const alpgpu::DecodeOptions opt {vpw, pad, ra, ser != 0, plain != 0};
		const alpgpu::ColumnSizes   sizes {n, packed, exc, alpgpu::policy_rd_vectors_of_hint(rd_hint)}; // (as api_decode.hip: planned)
		const alpgpu::DecodePlan    plan = alpgpu::policy_decode_plan(sizes, vb, opt);
		int                         kind = -1, shape = 0, ahead = 0;
		alpgpu::ReadAheadPace       pace {0, 0, 0};
		if (n != 0) { // (a stretch, an unhinted column and a column that is read ahead have vectors)
			kind = alpgpu::policy_stretch_kind(n, packed, exc, vb);
			// (as api_decode.hip: decode_unhinted hands the option to k_unhinted_plan)
			const alpgpu::UnhintedChoice c = alpgpu::policy_unhinted(n, static_cast<double>(packed), static_cast<double>(exceptions), static_cast<double>(rd_vectors), vb, (ra < 0 && ser) ? 0 : ra);
			shape = c.shape, ahead = c.ahead ? 1 : 0;
			pace  = alpgpu::policy_read_ahead_pace(static_cast<double>(n), static_cast<double>(packed), static_cast<double>(exc), vb, lead_us);
		}
		printf("%" PRIu64 " %d %d %d %d %d %u %u %u\n", alpgpu::decode_debug_word(plan.shape, vb), alpgpu::decode_shape_number(plan.shape), plan.ahead ? 1 : 0, kind, shape, ahead, pace.lead_min,
		       pace.lead_max, pace.ps_per_vector);
	}
	return 0;
}
