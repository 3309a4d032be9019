// blob_check.hpp — what bytes from outside must satisfy before a decode kernel may follow them: the rules of a serialized column's header, of one vector
// descriptor, and of the stream windows of the chunked host route (include/alpgpu.h: alpgpu_column_from_blob, alpgpu_decompress_host_*, alpgpu_column_validate).
// Plain C++ without a HIP type, like decode_policy.hpp's rule and persistent_launch.hpp: tests/cpp/blob_check_test.cpp includes it under g++ (and under the
// host sanitizers) and tests/blob_replica.py states the same rules in Python integers.  The host validator (api_container.hip: validate_blob_header /
// validate_blob_vectors), the chunked route (api_host.hip: decompress_host_range) and the device validator (guard_kernels.hip: k_validate_column) all
// take their verdicts from here; what stays with each caller is the scan of a record's exception positions, whose bytes live in host memory for one and
// in HBM for the other.
//
// No expression below can wrap for any field value: counts are compared by division, sums are formed only of terms already bounded, and differences only
// where the subtrahend has been compared first.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/alpgpu.h"

#if defined(__HIPCC__)
#define ALPGPU_BLOB_RULE __host__ __device__
#else
#define ALPGPU_BLOB_RULE
#endif

namespace alpgpu {

// A verdict: kBlobOk, or the first rule broken in the order the checks run (header before vectors; per vector: scheme, field, extent, window, position)
enum BlobRule : int {
	kBlobOk = 0,
	kBlobShort,        // header: size < 64
	kBlobIdentity,     // header: magic, version, header_bytes
	kBlobValueType,    // header: reserved names the other value type (or none)
	kBlobInconsistent, // header: n_rowgroups != ceil(n_vectors / 100), or n_values not inside the last vector
	kBlobTruncated,    // header: a stream beyond 2^56 bytes, or the blob's size beyond `size`
	kBlobScheme,       // descriptor: neither ALP nor ALP_RD, or not its rowgroup's scheme
	kBlobField,        // descriptor: a width, e / f or the exception count out of range
	kBlobExtent,       // descriptor: a record misaligned or not inside its stream
	kBlobWindowOrder,  // chunked route: the offsets at the chunks' first vectors do not ascend
	kBlobWindowRecord, // chunked route: a non-empty record outside its chunk's stream ranges
	kBlobPosition,     // an exception position >= 1024
};

constexpr uint64_t kBlobRowgroup  = 100;
constexpr uint64_t kBlobStreamMax = 1ull << 56;
constexpr uint32_t kBlobRecord    = 32; // sizeof(alpgpu_rowgroup_state) == sizeof(alpgpu_vector_desc)

ALPGPU_BLOB_RULE inline uint64_t blob_align8(uint64_t x) { return (x + 7ull) & ~7ull; } // x <= 2^64 - 8

// ---- the header --------------------------------------------------------------------------------------------------------------------------------------
// h_blob[0 .. size) -> h (a copy of the first 64 bytes when size allows).  kBlobOk promises: the rowgroup states, the descriptors and both streams, laid
// out behind the header as the fields say, lie inside [h_blob, h_blob + size).
inline BlobRule blob_check_header(const void* h_blob, uint64_t size, uint64_t value_bytes, alpgpu_blob_header& h) {
	if (size < sizeof(alpgpu_blob_header)) { return kBlobShort; }
	memcpy(&h, h_blob, sizeof(h));
	if (memcmp(h.magic, "ALPGPU1", 8) != 0 || h.version != 1 || h.header_bytes != sizeof(h)) { return kBlobIdentity; }
	if ((h.reserved == 0 ? 8ull : h.reserved) != value_bytes) { return kBlobValueType; }
	// ceil(x / m) as x / m + (x % m != 0): x + m - 1 wraps for x near 2^64, and so does n_vectors * 1024
	if (h.n_rowgroups != h.n_vectors / kBlobRowgroup + (h.n_vectors % kBlobRowgroup != 0 ? 1 : 0)) { return kBlobInconsistent; }
	if (h.n_vectors != h.n_values / 1024 + (h.n_values % 1024 != 0 ? 1 : 0)) { return kBlobInconsistent; } // n_values in ((n - 1) * 1024, n * 1024]; 0 for n = 0
	if (h.packed_bytes > kBlobStreamMax || h.exc_bytes > kBlobStreamMax) { return kBlobTruncated; }
	const uint64_t body = size - sizeof(alpgpu_blob_header);
	if (h.n_vectors > body / kBlobRecord) { return kBlobTruncated; } // from here on n_vectors < 2^59: the sum below stays under 2^61
	const uint64_t need = kBlobRecord * h.n_rowgroups + kBlobRecord * h.n_vectors + blob_align8(h.packed_bytes) + blob_align8(h.exc_bytes);
	return need > body ? kBlobTruncated : kBlobOk;
}

// ---- one descriptor ------------------------------------------------------------------------------------------------------------------------------------
ALPGPU_BLOB_RULE inline uint64_t blob_packed_size(const alpgpu_vector_desc& d) { return 128ull * (d.bw + (d.scheme == ALPGPU_SCHEME_ALP_RD ? d.lbw : 0u)); }
ALPGPU_BLOB_RULE inline uint64_t blob_exc_value_bytes(const alpgpu_vector_desc& d, uint32_t value_bytes) { return d.scheme == ALPGPU_SCHEME_ALP ? value_bytes : 2u; }
ALPGPU_BLOB_RULE inline uint64_t blob_exc_size(const alpgpu_vector_desc& d, uint32_t value_bytes) {
	return blob_align8((blob_exc_value_bytes(d, value_bytes) + 2ull) * d.exc_cnt); // values, then 2-byte positions, rounded up to 8
}

// d against its rowgroup's state rg and the two streams' sizes (a blob's packed_bytes / exc_bytes, a device column's capacities): kBlobOk, or kBlobScheme,
// kBlobField or kBlobExtent.  Fields the header documents as unused for the vector's scheme (an ALP vector's lbw; an ALP_RD vector's e, f and base) are
// not looked at: no kernel reads them for that scheme.  kBlobOk promises that the packed words and the exception record lie inside the streams.
ALPGPU_BLOB_RULE inline BlobRule blob_check_descriptor(const alpgpu_vector_desc& d, const alpgpu_rowgroup_state& rg, uint32_t value_bytes, uint64_t packed_bytes,
                                                       uint64_t exc_bytes) {
	const uint32_t vbits = 8u * value_bytes;         // 64 or 32
	const uint32_t max_e = value_bytes == 8 ? 18u : 10u;
	const bool     alp = d.scheme == ALPGPU_SCHEME_ALP, rd = d.scheme == ALPGPU_SCHEME_ALP_RD;
	if ((!alp && !rd) || rg.scheme != d.scheme) { return kBlobScheme; }
	if (d.bw > vbits || d.exc_cnt > 1024) { return kBlobField; }
	if (alp && (d.e > max_e || d.f > d.e)) { return kBlobField; }
	if (rd && (d.lbw < 1 || d.lbw > 3 || d.bw > vbits - 1 || d.bw != rg.rd_rbw || d.lbw != rg.rd_lbw)) { return kBlobField; }
	if ((d.packed_off & 127ull) != 0 || (d.exc_off & 7ull) != 0) { return kBlobExtent; }
	if (d.packed_off > packed_bytes || blob_packed_size(d) > packed_bytes - d.packed_off) { return kBlobExtent; }
	if (d.exc_off > exc_bytes || blob_exc_size(d, value_bytes) > exc_bytes - d.exc_off) { return kBlobExtent; }
	return kBlobOk;
}

// ---- the chunked route's windows -------------------------------------------------------------------------------------------------------------------------
// The host route uploads the streams chunk by chunk: while chunk c of a range [v_begin, v_end) of vectors is decoded, HBM holds the stream bytes from the
// offsets of the chunk's first vector to those of the next chunk's first vector (the streams' ends behind the column's last vector).
struct BlobWindow {
	uint64_t w[4]; // packed [w[0], w[1]), exceptions [w[2], w[3])
	bool     ok;   // the range's and the chunk's offsets ascend and stay inside the streams
};

inline alpgpu_vector_desc blob_desc_at(const void* descs, uint64_t v) {
	alpgpu_vector_desc d;
	memcpy(&d, static_cast<const uint8_t*>(descs) + kBlobRecord * v, sizeof(d));
	return d;
}

// descs: the blob's n descriptors (any alignment).  The whole range's extents come out as chunk 0 of a chunk length of v_end - v_begin.
inline BlobWindow blob_chunk_window(const void* descs, uint64_t n, uint64_t packed_bytes, uint64_t exc_bytes, uint64_t v_begin, uint64_t v_end, uint64_t chunk,
                                    uint64_t c) {
	const uint64_t P0 = blob_desc_at(descs, v_begin).packed_off, E0 = blob_desc_at(descs, v_begin).exc_off;
	const uint64_t P1 = v_end < n ? blob_desc_at(descs, v_end).packed_off : packed_bytes;
	const uint64_t E1 = v_end < n ? blob_desc_at(descs, v_end).exc_off : exc_bytes;
	const uint64_t v0 = v_begin + c * chunk, v1 = v_end - v0 < chunk ? v_end : v0 + chunk;
	BlobWindow     W;
	W.w[0] = blob_desc_at(descs, v0).packed_off, W.w[2] = blob_desc_at(descs, v0).exc_off;
	W.w[1] = v1 < n ? blob_desc_at(descs, v1).packed_off : packed_bytes;
	W.w[3] = v1 < n ? blob_desc_at(descs, v1).exc_off : exc_bytes;
	W.ok   = P0 <= P1 && E0 <= E1 && P1 <= packed_bytes && E1 <= exc_bytes && P0 <= W.w[0] && W.w[0] <= W.w[1] && W.w[1] <= P1 && E0 <= W.w[2] && W.w[2] <= W.w[3] &&
	       W.w[3] <= E1;
	return W;
}

// a descriptor that passed blob_check_descriptor against its chunk's window: an empty record is nowhere, so it is inside any window
ALPGPU_BLOB_RULE inline bool blob_record_in_window(const alpgpu_vector_desc& d, uint32_t value_bytes, const uint64_t* w) {
	const uint64_t psz = blob_packed_size(d), esz = blob_exc_size(d, value_bytes);
	return (psz == 0 || (d.packed_off >= w[0] && d.packed_off + psz <= w[1])) && (esz == 0 || (d.exc_off >= w[2] && d.exc_off + esz <= w[3]));
}

// ---- the vectors of a blob in host memory ------------------------------------------------------------------------------------------------------------------
// Vectors [v_begin, v_end) of a blob whose header passed blob_check_header: every extent a kernel will dereference is checked here, so a corrupt blob cannot
// make the decoder read out of bounds.  window (optional) = BlobWindow::w of the chunk these vectors are decoded in.  *first_bad (optional) = the vector
// at which the scan stopped.
inline BlobRule blob_check_vectors(const void* h_blob, const alpgpu_blob_header& h, uint32_t value_bytes, uint64_t v_begin, uint64_t v_end, const uint64_t* window,
                                   uint64_t* first_bad) {
	const uint8_t* rgs  = static_cast<const uint8_t*>(h_blob) + sizeof(h);
	const uint8_t* vds  = rgs + kBlobRecord * h.n_rowgroups;
	const uint8_t* excs = vds + kBlobRecord * h.n_vectors + blob_align8(h.packed_bytes);
	for (uint64_t v = v_begin; v < v_end; ++v) {
		if (first_bad) { *first_bad = v; }
		const alpgpu_vector_desc d = blob_desc_at(vds, v);
		alpgpu_rowgroup_state    rg;
		memcpy(&rg, rgs + kBlobRecord * (v / kBlobRowgroup), sizeof(rg));
		if (const BlobRule r = blob_check_descriptor(d, rg, value_bytes, h.packed_bytes, h.exc_bytes)) { return r; }
		if (window != nullptr && !blob_record_in_window(d, value_bytes, window)) { return kBlobWindowRecord; }
		// only now is the record known to lie inside the stream.  Positions are 16-bit: OR them and look at the bits above 1023 once
		const uint8_t* pos = excs + d.exc_off + blob_exc_value_bytes(d, value_bytes) * d.exc_cnt;
		uint32_t       any = 0;
		for (uint32_t j = 0; j < d.exc_cnt; ++j) {
			uint16_t q;
			memcpy(&q, pos + 2u * j, 2);
			any |= q;
		}
		if (any >= 1024) { return kBlobPosition; }
	}
	if (first_bad) { *first_bad = ~0ull; }
	return kBlobOk;
}

} // namespace alpgpu
