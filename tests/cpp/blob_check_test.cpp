// CPU driver of alp_amd/csrc/blob_check.hpp for tests/test_blob_check_cpu.py: the header rule, the per-descriptor rule with the host's position scan, and the
// chunk windows, run over the blobs it is fed.  Plain C++ (g++ -std=c++17 -Wall -Werror, and once more with -fsanitize=address,undefined): no HIP, no GPU.
//
// Standard input = the cases, each: u64 size, u64 value_bytes, u64 chunk, u64 n_ranges, n_ranges x (u64 v_begin, u64 v_end), then `size` bytes of blob.  Every
// case is copied into a heap buffer of EXACTLY `size` bytes, so that under AddressSanitizer a read one byte past what the caller handed over ends the run.
// chunk = 0: the one-piece route (validate the header, then every vector against the whole streams).  chunk > 0: the chunked host route over each range in
// turn, as decompress_host_range walks it: the range's extents, then chunk by chunk its window and its vectors.
// One line per case: "accept - -", or "refuse <rule> <first bad vector or ->".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blob_check.hpp"

using namespace alpgpu;

static const char* rule_name(BlobRule r) {
	switch (r) {
	case kBlobOk: return "ok";
	case kBlobShort: return "short";
	case kBlobIdentity: return "identity";
	case kBlobValueType: return "type";
	case kBlobInconsistent: return "inconsistent";
	case kBlobTruncated: return "truncated";
	case kBlobScheme: return "scheme";
	case kBlobField: return "field";
	case kBlobExtent: return "extent";
	case kBlobWindowOrder: return "order";
	case kBlobWindowRecord: return "record";
	case kBlobPosition: return "position";
	}
	return "?";
}

static bool read_u64(FILE* f, uint64_t* x) { return fread(x, 8, 1, f) == 1; }

static void refuse(BlobRule r, uint64_t v) { printf("refuse %s %llu\n", rule_name(r), static_cast<unsigned long long>(v)); }

int main() {
	FILE* f = stdin;
	uint64_t size, value_bytes, chunk, n_ranges;
	while (read_u64(f, &size)) {
		if (!read_u64(f, &value_bytes) || !read_u64(f, &chunk) || !read_u64(f, &n_ranges)) { return 3; }
		std::vector<uint64_t> ranges(2 * n_ranges);
		for (auto& x : ranges) {
			if (!read_u64(f, &x)) { return 3; }
		}
		uint8_t* blob = static_cast<uint8_t*>(malloc(size));
		if (size && (!blob || fread(blob, 1, size, f) != size)) { return 3; }
		alpgpu_blob_header h;
		const BlobRule     hr = blob_check_header(blob, size, value_bytes, h);
		if (hr != kBlobOk) {
			printf("refuse %s -\n", rule_name(hr));
		} else if (chunk == 0) {
			uint64_t       bad = 0;
			const BlobRule r   = blob_check_vectors(blob, h, static_cast<uint32_t>(value_bytes), 0, h.n_vectors, nullptr, &bad);
			r == kBlobOk ? static_cast<void>(printf("accept - -\n")) : refuse(r, bad);
		} else {
			const uint8_t* descs = blob + sizeof(h) + kBlobRecord * h.n_rowgroups;
			bool           done  = false;
			for (uint64_t i = 0; i < n_ranges && !done; ++i) {
				const uint64_t v_begin = ranges[2 * i], v_end = ranges[2 * i + 1];
				if (v_begin >= v_end) { continue; }
				if (!blob_chunk_window(descs, h.n_vectors, h.packed_bytes, h.exc_bytes, v_begin, v_end, v_end - v_begin, 0).ok) {
					refuse(kBlobWindowOrder, v_begin), done = true;
					break;
				}
				const uint64_t n_chunks = (v_end - v_begin + chunk - 1) / chunk;
				for (uint64_t c = 0; c < n_chunks && !done; ++c) {
					const uint64_t   v0 = v_begin + c * chunk, v1 = v_end - v0 < chunk ? v_end : v0 + chunk;
					const BlobWindow W = blob_chunk_window(descs, h.n_vectors, h.packed_bytes, h.exc_bytes, v_begin, v_end, chunk, c);
					if (!W.ok) {
						refuse(kBlobWindowOrder, v0), done = true;
						break;
					}
					uint64_t       bad = 0;
					const BlobRule r   = blob_check_vectors(blob, h, static_cast<uint32_t>(value_bytes), v0, v1, W.w, &bad);
					if (r != kBlobOk) { refuse(r, bad), done = true; }
				}
			}
			if (!done) { printf("accept - -\n"); }
		}
		free(blob);
	}
	return 0;
}
