// alp/batch.hpp — the reference's per-vector loop, a rowgroup at a time.
//
// The per-vector functions of this header set (alp::encoder<PT>::encode, analyze_ffor, ffor::ffor, falp, patch_exceptions)
// ship ONE 1024-value vector to the GPU and back per call: 2 uploads, 1-3 kernels and 4-5 synchronous downloads per vector,
// bound by PCIe round trips (INTEGRATION.md has the measured rates).  A caller that keeps the reference's loop shape
//
//     for each rowgroup:  encoder::init(...)                                  (include/alp/encoder.hpp:402-427 upstream,
//         for each vector:  encoder::encode(...); analyze_ffor(...); ffor(...)  test/test_alp_sample.cpp:137-166)
//
// replaces the inner loop by ONE call of alp::gpu::rowgroup<PT>::encode (and the decode loop falp + patch_exceptions by
// ::decode): one upload, three kernels over all vectors of the rowgroup, one download — literally one copy each way: the arrays of
// a call lie next to each other in one device buffer and in a page-locked host mirror of it.  The outputs are the per-vector
// outputs of the reference, at a fixed stride of 1024 elements per vector: the FFOR-packed words (16 * bit_width words
// used), bit widths, bases, (factor, exponent), exceptions, positions, counts.  Bit-identical to calling the per-vector
// functions in a loop (tests/cpp/batch_test.cpp checks that on the GPU).  ALP_RD rowgroups have ::encode_rd / ::decode_rd.
#ifndef ALP_BATCH_HPP
#define ALP_BATCH_HPP
#include <algorithm>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <mutex>
#include <utility>
#include <vector>

#include "alp/config.hpp"
#include "alp/decoder.hpp"
#include "alp/encoder.hpp"
#include "alp/gpu_bridge.hpp"

namespace alp { namespace gpu {

// Per-thread scratch of the batched calls: one device buffer and a page-locked host mirror of it.  Every call lays the arrays it
// needs out next to each other (sized for ITS n vectors), so that whatever goes up is one contiguous copy and whatever comes
// down is another; user arrays are copied into / out of the mirror with memcpy.
//   [ idx: cap x u32 zeros (every vector uses state 0) ][ state: 64 B ][ the call's arrays ... ]
struct batch_scratch {
	uint8_t* dev {nullptr};
	uint8_t* host {nullptr};
	size_t   cap {0};   // vectors the zero index array covers
	size_t   bytes {0}; // size of both buffers
	~batch_scratch() {
		if (dev) { alpgpu_free(context(), dev); }
		if (host) { alpgpu_free_host(context(), host); }
	}
	size_t off_state() const { return (cap * 4 + 63) & ~size_t(63); }
	size_t off_arrays() const { return off_state() + 64; }
	// room for n vectors whose arrays take at most per_vector bytes each
	void ensure(size_t n, size_t per_vector) {
		const size_t want_cap = n < 100 ? 100 : n;
		const size_t need     = ((want_cap * 4 + 63) & ~size_t(63)) + 64 + want_cap * per_vector + 64;
		if (want_cap <= cap && need <= bytes) { return; }
		if (dev) { check(alpgpu_free(context(), dev), "alpgpu_free"); }
		if (host) { check(alpgpu_free_host(context(), host), "alpgpu_free_host"); }
		dev = host = nullptr;
		cap   = want_cap > cap ? want_cap : cap;
		bytes = ((cap * 4 + 63) & ~size_t(63)) + 64 + cap * per_vector + 64;
		if (bytes < need) { bytes = need; }
		check(alpgpu_malloc(context(), reinterpret_cast<void**>(&dev), bytes), "alpgpu_malloc");
		check(alpgpu_malloc_host(context(), reinterpret_cast<void**>(&host), bytes), "alpgpu_malloc_host");
		check(alpgpu_memset(context(), dev, 0, off_state()), "alpgpu_memset");
	}
	template <class T>
	T* d(size_t off) const {
		return reinterpret_cast<T*>(dev + off);
	}
	uint8_t* h(size_t off) const { return host + off; }
	void     up(size_t off, size_t n) const { check(alpgpu_memcpy_h2d_async(context(), dev + off, host + off, n), "alpgpu_memcpy_h2d_async"); }
	void     down(size_t off, size_t n) const { check(alpgpu_memcpy_d2h(context(), host + off, dev + off, n), "alpgpu_memcpy_d2h"); } // synchronous
};
inline batch_scratch& batch_tls() {
	static thread_local batch_scratch s;
	return s;
}

template <class PT>
struct rowgroup {
	using ST = typename inner_t<PT>::st;
	using UT = typename inner_t<PT>::ut;
	static constexpr size_t V  = config::VECTOR_SIZE;
	static constexpr size_t VB = V * sizeof(PT); // bytes of one vector of values / encoded integers / right parts

	// the arrays of the ALP calls, in the order they lie in the buffers (n = vectors of this call)
	struct alp_layout {
		size_t in, exc, packed, pos, base, cnt, bw, fac, exp, enc, end;
		alp_layout(const batch_scratch& s, size_t n) {
			in     = s.off_arrays();       // n x VB   values in (encode) / out (decode)
			exc    = in + n * VB;          // n x VB   exception values            -+
			packed = exc + n * VB;         // n x VB   FFOR words                    |
			pos    = packed + n * VB;      // n x 2 KiB exception positions         |  one block: encode's output,
			base   = pos + n * 2048;       // n x 8                                 |  decode's input
			cnt    = base + n * 8;         // n x 2                                 |
			bw     = cnt + n * 2;          // n                                     |
			fac    = bw + n;               // n                                     |
			exp    = fac + n;              // n                                    -+
			enc    = (exp + n + 15) & ~size_t(15); // n x VB   encoded integers (device only)
			end    = enc + n * VB;
		}
	};
	static constexpr size_t kAlpPerVector = 4 * VB + 2048 + 8 + 2 + 3 + 1;
	// ... and of the ALP_RD calls
	struct rd_layout {
		size_t in, right, left, exc, pos, cnt, end;
		rd_layout(const batch_scratch& s, size_t n) {
			in    = s.off_arrays();   // n x VB    values in (encode) / out (decode)
			right = in + n * VB;      // n x VB    right parts          -+
			left  = right + n * VB;   // n x 2 KiB dictionary indices    |  one block: encode's output, decode's input
			exc   = left + n * 2048;  // n x 2 KiB exceptions            |
			pos   = exc + n * 2048;   // n x 2 KiB positions             |
			cnt   = pos + n * 2048;   // n x 2                          -+
			end   = cnt + n * 2;
		}
	};
	static constexpr size_t kRdPerVector = 2 * VB + 3 * 2048 + 2 + 1;
	static constexpr size_t kPerVector   = kAlpPerVector > kRdPerVector ? kAlpPerVector : kRdPerVector;

	//! ALP rowgroup: second-level sampling + encode, analyze_ffor, ffor for n_vectors vectors sharing `stt` (from encoder<PT>::init).
	//! All outputs are host arrays at a stride of 1024 elements per vector (counts / bit_widths / bases / facs / exps: one per vector).
	static void encode(const PT* vectors, size_t n_vectors, const state<PT>& stt, ST* ffor_packed, bw_t* bit_widths, ST* bases, uint8_t* facs, uint8_t* exps,
	                   PT* exceptions, exp_p_t* positions, exp_c_t* counts) {
		if (n_vectors == 0) { return; }
		auto& s = batch_tls();
		s.ensure(n_vectors, kPerVector);
		alpgpu_ctx*                 c = context();
		const alpgpu_rowgroup_state d = to_device_state(stt);
		const uint64_t              n = n_vectors;
		const alp_layout            L(s, n);
		std::memcpy(s.h(s.off_state()), &d, sizeof(d));
		std::memcpy(s.h(L.in), vectors, n * VB);
		s.up(s.off_state(), L.in + n * VB - s.off_state()); // state + values: one copy
		auto* st  = s.d<alpgpu_rowgroup_state>(s.off_state());
		auto* idx = s.d<uint32_t>(0);
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_encode_values_f64(c, s.d<double>(L.in), st, idx, s.d<double>(L.exc), s.d<uint16_t>(L.pos), V, s.d<uint16_t>(L.cnt), s.d<int64_t>(L.enc),
			                               s.d<uint8_t>(L.fac), s.d<uint8_t>(L.exp), n), "alpgpu_encode_values_f64");
			check(alpgpu_analyze_ffor_i64(c, s.d<int64_t>(L.enc), s.d<uint8_t>(L.bw), s.d<int64_t>(L.base), n), "alpgpu_analyze_ffor_i64");
			check(alpgpu_ffor_i64(c, s.d<int64_t>(L.enc), s.d<int64_t>(L.packed), V, s.d<uint8_t>(L.bw), s.d<int64_t>(L.base), n), "alpgpu_ffor_i64");
		} else {
			check(alpgpu_encode_values_f32(c, s.d<float>(L.in), st, idx, s.d<float>(L.exc), s.d<uint16_t>(L.pos), V, s.d<uint16_t>(L.cnt), s.d<int32_t>(L.enc),
			                               s.d<uint8_t>(L.fac), s.d<uint8_t>(L.exp), n), "alpgpu_encode_values_f32");
			check(alpgpu_analyze_ffor_i32(c, s.d<int32_t>(L.enc), s.d<uint8_t>(L.bw), s.d<int32_t>(L.base), n), "alpgpu_analyze_ffor_i32");
			check(alpgpu_ffor_i32(c, s.d<int32_t>(L.enc), s.d<int32_t>(L.packed), V, s.d<uint8_t>(L.bw), s.d<int32_t>(L.base), n), "alpgpu_ffor_i32");
		}
		s.down(L.exc, L.exp + n - L.exc); // everything the caller gets back: one copy
		std::memcpy(exceptions, s.h(L.exc), n * VB);
		std::memcpy(ffor_packed, s.h(L.packed), n * VB);
		std::memcpy(positions, s.h(L.pos), n * 2048);
		// bases travel as 8 bytes per vector; the float API's are int32
		if constexpr (sizeof(ST) == 8) {
			std::memcpy(bases, s.h(L.base), n * 8);
		} else {
			std::memcpy(bases, s.h(L.base), n * 4);
		}
		std::memcpy(counts, s.h(L.cnt), n * 2);
		std::memcpy(bit_widths, s.h(L.bw), n);
		std::memcpy(facs, s.h(L.fac), n);
		std::memcpy(exps, s.h(L.exp), n);
	}

	//! falp + patch_exceptions for n_vectors vectors (inputs as produced by encode())
	static void decode(const ST* ffor_packed, const bw_t* bit_widths, const ST* bases, const uint8_t* facs, const uint8_t* exps, const PT* exceptions,
	                   const exp_p_t* positions, const exp_c_t* counts, size_t n_vectors, PT* out) {
		if (n_vectors == 0) { return; }
		auto& s = batch_tls();
		s.ensure(n_vectors, kPerVector);
		alpgpu_ctx*      c = context();
		const uint64_t   n = n_vectors;
		const alp_layout L(s, n);
		std::memcpy(s.h(L.exc), exceptions, n * VB);
		std::memcpy(s.h(L.packed), ffor_packed, n * VB);
		std::memcpy(s.h(L.pos), positions, n * 2048);
		std::memcpy(s.h(L.base), bases, n * sizeof(ST));
		std::memcpy(s.h(L.cnt), counts, n * 2);
		std::memcpy(s.h(L.bw), bit_widths, n);
		std::memcpy(s.h(L.fac), facs, n);
		std::memcpy(s.h(L.exp), exps, n);
		s.up(L.exc, L.exp + n - L.exc); // one copy
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_falp_f64(c, s.d<int64_t>(L.packed), V, s.d<double>(L.in), s.d<uint8_t>(L.bw), s.d<int64_t>(L.base), s.d<uint8_t>(L.fac), s.d<uint8_t>(L.exp), n),
			      "alpgpu_falp_f64");
			check(alpgpu_patch_f64(c, s.d<double>(L.in), s.d<double>(L.exc), s.d<uint16_t>(L.pos), V, s.d<uint16_t>(L.cnt), n), "alpgpu_patch_f64");
		} else {
			check(alpgpu_falp_f32(c, s.d<int32_t>(L.packed), V, s.d<float>(L.in), s.d<uint8_t>(L.bw), s.d<int32_t>(L.base), s.d<uint8_t>(L.fac), s.d<uint8_t>(L.exp), n),
			      "alpgpu_falp_f32");
			check(alpgpu_patch_f32(c, s.d<float>(L.in), s.d<float>(L.exc), s.d<uint16_t>(L.pos), V, s.d<uint16_t>(L.cnt), n), "alpgpu_patch_f32");
		}
		s.down(L.in, n * VB);
		std::memcpy(out, s.h(L.in), n * VB);
	}

	//! ALP_RD rowgroup (rd_encoder<PT>::encode per vector, include/alp/rd.hpp:109-147 upstream): right parts, left dictionary
	//! indices, exceptions (left parts), positions, counts — unpacked, at a stride of 1024 per vector, as the reference returns them
	static void encode_rd(const PT* vectors, size_t n_vectors, const state<PT>& stt, UT* right_parts, uint16_t* left_parts, uint16_t* exceptions, exp_p_t* positions,
	                      exp_c_t* counts) {
		if (n_vectors == 0) { return; }
		auto& s = batch_tls();
		s.ensure(n_vectors, kPerVector);
		alpgpu_ctx*                 c = context();
		const alpgpu_rowgroup_state d = to_device_state(stt);
		const uint64_t              n = n_vectors;
		const rd_layout             L(s, n);
		std::memcpy(s.h(s.off_state()), &d, sizeof(d));
		std::memcpy(s.h(L.in), vectors, n * VB);
		s.up(s.off_state(), L.in + n * VB - s.off_state());
		auto* st  = s.d<alpgpu_rowgroup_state>(s.off_state());
		auto* idx = s.d<uint32_t>(0);
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_rd_encode_vectors_f64(c, s.d<double>(L.in), st, idx, s.d<uint16_t>(L.exc), s.d<uint16_t>(L.pos), V, s.d<uint16_t>(L.cnt), s.d<uint64_t>(L.right),
			                                   s.d<uint16_t>(L.left), n), "alpgpu_rd_encode_vectors_f64");
		} else {
			check(alpgpu_rd_encode_vectors_f32(c, s.d<float>(L.in), st, idx, s.d<uint16_t>(L.exc), s.d<uint16_t>(L.pos), V, s.d<uint16_t>(L.cnt), s.d<uint32_t>(L.right),
			                                   s.d<uint16_t>(L.left), n), "alpgpu_rd_encode_vectors_f32");
		}
		s.down(L.right, L.cnt + n * 2 - L.right);
		std::memcpy(right_parts, s.h(L.right), n * VB);
		std::memcpy(left_parts, s.h(L.left), n * 2048);
		std::memcpy(exceptions, s.h(L.exc), n * 2048);
		std::memcpy(positions, s.h(L.pos), n * 2048);
		std::memcpy(counts, s.h(L.cnt), n * 2);
	}

	//! rd_encoder<PT>::decode per vector (rd.hpp:152-178 upstream) for n_vectors vectors
	static void decode_rd(const UT* right_parts, const uint16_t* left_parts, const uint16_t* exceptions, const exp_p_t* positions, const exp_c_t* counts,
	                      const state<PT>& stt, size_t n_vectors, PT* out) {
		if (n_vectors == 0) { return; }
		auto& s = batch_tls();
		s.ensure(n_vectors, kPerVector);
		alpgpu_ctx*                 c = context();
		const alpgpu_rowgroup_state d = to_device_state(stt);
		const uint64_t              n = n_vectors;
		const rd_layout             L(s, n);
		std::memcpy(s.h(s.off_state()), &d, sizeof(d));
		std::memcpy(s.h(L.right), right_parts, n * VB);
		std::memcpy(s.h(L.left), left_parts, n * 2048);
		std::memcpy(s.h(L.exc), exceptions, n * 2048);
		std::memcpy(s.h(L.pos), positions, n * 2048);
		std::memcpy(s.h(L.cnt), counts, n * 2);
		s.up(s.off_state(), 64);
		s.up(L.right, L.cnt + n * 2 - L.right);
		auto* st  = s.d<alpgpu_rowgroup_state>(s.off_state());
		auto* idx = s.d<uint32_t>(0);
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_rd_decode_vectors_f64(c, s.d<double>(L.in), s.d<uint64_t>(L.right), s.d<uint16_t>(L.left), st, idx, s.d<uint16_t>(L.exc), s.d<uint16_t>(L.pos), V,
			                                   s.d<uint16_t>(L.cnt), n), "alpgpu_rd_decode_vectors_f64");
		} else {
			check(alpgpu_rd_decode_vectors_f32(c, s.d<float>(L.in), s.d<uint32_t>(L.right), s.d<uint16_t>(L.left), st, idx, s.d<uint16_t>(L.exc), s.d<uint16_t>(L.pos), V,
			                                   s.d<uint16_t>(L.cnt), n), "alpgpu_rd_decode_vectors_f32");
		}
		s.down(L.in, n * VB);
		std::memcpy(out, s.h(L.in), n * VB);
	}
};

// A whole column that lives in host memory, to and from its serialized form (include/alpgpu.h: alpgpu_compress_host_* — chunks of whole
// rowgroups go up on one stream while the previous chunk is encoded on another; ~35 GB/s of doubles from page-locked memory, ~10 GB/s
// from pageable memory like the std::vectors used here; callers that care hand page-locked buffers to the C functions directly).
// This is what replaces the reference's caller loop (publication/source_code/bench_compression_ratio/alp.cpp:198-229) as a whole.
// A pool of contexts for a list of devices (one each; the same device may be listed more than once — e.g. in tests on a one-GPU box):
// what alp::gpu::column<PT>::compress / decompress over a device list run on.  Contexts live until the process ends.
// A context serves ONE pipeline at a time (include/alpgpu.h: "a context must not be used by anything else during the call"), so the pool
// hands contexts out as a LEASE: entries are marked in use until the lease is destroyed, and a second thread that asks for the same devices
// meanwhile gets other (new) contexts.  column<PT>::compress / decompress over a device list are thereby safe to call from several threads.
struct context_pool {
	struct entry {
		int         device;
		alpgpu_ctx* ctx;
		bool        in_use;
	};
	std::mutex         mu;
	std::vector<entry> entries; // in creation order; contexts live until the process ends
	static context_pool& instance() {
		static context_pool p;
		return p;
	}
};
class context_lease {
	std::vector<alpgpu_ctx*> ctxs_;
	std::vector<size_t>      held_;

public:
	explicit context_lease(const std::vector<int>& devices) {
		context_pool&               P = context_pool::instance();
		std::lock_guard<std::mutex> lock(P.mu);
		try {
			for (int dev : devices) {
				size_t at = P.entries.size();
				for (size_t i = 0; i < P.entries.size(); ++i) {
					if (!P.entries[i].in_use && P.entries[i].device == dev) {
						at = i;
						break;
					}
				}
				if (at == P.entries.size()) {
					alpgpu_ctx* c = nullptr;
					check(alpgpu_ctx_create(dev, &c), "alpgpu_ctx_create");
					P.entries.push_back({dev, c, false});
				}
				P.entries[at].in_use = true;
				held_.push_back(at);
				ctxs_.push_back(P.entries[at].ctx);
			}
		} catch (...) {
			for (size_t i : held_) { P.entries[i].in_use = false; }
			throw;
		}
	}
	~context_lease() {
		context_pool&               P = context_pool::instance();
		std::lock_guard<std::mutex> lock(P.mu);
		for (size_t i : held_) { P.entries[i].in_use = false; }
	}
	context_lease(const context_lease&)            = delete;
	context_lease& operator=(const context_lease&) = delete;
	const std::vector<alpgpu_ctx*>& contexts() const { return ctxs_; }
};

template <class PT>
struct column {
	// The column cut into whole-rowgroup shards over `devices` (alpgpu_compress_host_multi_*): every GPU of the node works on its shard
	// over its own PCIe link, the result is the one-device blob byte for byte.
	static std::vector<uint8_t> compress(const PT* values, size_t n_values, const std::vector<int>& devices) {
		const context_lease             lease(devices); // the contexts are this call's until it returns
		const std::vector<alpgpu_ctx*>& ctxs = lease.contexts();
		const uint64_t                 n    = (n_values + config::VECTOR_SIZE - 1) / config::VECTOR_SIZE;
		uint64_t                       cap  = alpgpu_blob_size(n, n * config::VECTOR_SIZE * sizeof(PT) + 1024 * ctxs.size(), 0);
		std::vector<uint8_t>           blob;
		for (int attempt = 0; attempt < 2; ++attempt) {
			blob.resize(cap);
			uint64_t  written = 0;
			const int rc = sizeof(PT) == 8 ? alpgpu_compress_host_multi_f64(ctxs.data(), static_cast<int>(ctxs.size()), reinterpret_cast<const double*>(values), n_values, blob.data(), cap, &written)
			                               : alpgpu_compress_host_multi_f32(ctxs.data(), static_cast<int>(ctxs.size()), reinterpret_cast<const float*>(values), n_values, blob.data(), cap, &written);
			if (rc == ALPGPU_ERR_CAPACITY && attempt == 0 && written > cap) {
				cap = written;
				continue;
			}
			check(rc, "alpgpu_compress_host_multi");
			blob.resize(written);
			break;
		}
		return blob;
	}
	static std::vector<PT> decompress(const uint8_t* blob, size_t size, const std::vector<int>& devices) {
		const context_lease             lease(devices);
		const std::vector<alpgpu_ctx*>& ctxs = lease.contexts();
		uint64_t  n_values = 0;
		const int probe    = sizeof(PT) == 8 ? alpgpu_decompress_host_multi_f64(ctxs.data(), 1, blob, size, nullptr, 0, &n_values)
		                                     : alpgpu_decompress_host_multi_f32(ctxs.data(), 1, blob, size, nullptr, 0, &n_values);
		if (probe != ALPGPU_OK && probe != ALPGPU_ERR_CAPACITY) { check(probe, "alpgpu_decompress_host_multi (header)"); }
		std::vector<PT> out(n_values);
		if (n_values == 0) { return out; }
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_decompress_host_multi_f64(ctxs.data(), static_cast<int>(ctxs.size()), blob, size, reinterpret_cast<double*>(out.data()), out.size(), &n_values), "alpgpu_decompress_host_multi_f64");
		} else {
			check(alpgpu_decompress_host_multi_f32(ctxs.data(), static_cast<int>(ctxs.size()), blob, size, reinterpret_cast<float*>(out.data()), out.size(), &n_values), "alpgpu_decompress_host_multi_f32");
		}
		return out;
	}
	static std::vector<uint8_t> compress(const PT* values, size_t n_values) {
		const uint64_t n = (n_values + config::VECTOR_SIZE - 1) / config::VECTOR_SIZE;
		// a compressed column is almost never larger than the column: start there, and take the size the library asks for otherwise
		// (the worst case — every value an exception — is 2.3 times the input)
		uint64_t             cap = alpgpu_blob_size(n, n * config::VECTOR_SIZE * sizeof(PT) + 1024, 0);
		std::vector<uint8_t> blob;
		for (int attempt = 0; attempt < 2; ++attempt) {
			blob.resize(cap);
			uint64_t written = 0;
			const int rc = sizeof(PT) == 8 ? alpgpu_compress_host_f64(context(), reinterpret_cast<const double*>(values), n_values, blob.data(), cap, &written)
			                               : alpgpu_compress_host_f32(context(), reinterpret_cast<const float*>(values), n_values, blob.data(), cap, &written);
			if (rc == ALPGPU_ERR_CAPACITY && attempt == 0 && written > cap) {
				cap = written;
				continue;
			}
			check(rc, "alpgpu_compress_host");
			blob.resize(written);
			break;
		}
		return blob;
	}
	static std::vector<PT> decompress(const uint8_t* blob, size_t size) {
		// the value count comes from the library AFTER it has validated the header (a call with no output capacity returns it with
		// ALPGPU_ERR_CAPACITY): nothing is allocated on the word of a corrupt or hostile blob
		uint64_t n_values = 0;
		const int probe   = sizeof(PT) == 8 ? alpgpu_decompress_host_f64(context(), blob, size, nullptr, 0, &n_values)
		                                    : alpgpu_decompress_host_f32(context(), blob, size, nullptr, 0, &n_values);
		if (probe != ALPGPU_OK && probe != ALPGPU_ERR_CAPACITY) { check(probe, "alpgpu_decompress_host (header)"); }
		std::vector<PT> out(n_values);
		if (n_values == 0) { return out; }
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_decompress_host_f64(context(), blob, size, out.data(), out.size(), &n_values), "alpgpu_decompress_host_f64");
		} else {
			check(alpgpu_decompress_host_f32(context(), blob, size, out.data(), out.size(), &n_values), "alpgpu_decompress_host_f32");
		}
		return out;
	}
	// Device buffers freed with the object.  A type of its own: as a complete member (or local) its destructor also runs when the code that fills
	// it throws half way, a constructor of the owner included.
	struct device_buffers {
		std::vector<void*> p;
		device_buffers() = default;
		device_buffers(const device_buffers&)            = delete;
		device_buffers& operator=(const device_buffers&) = delete;
		~device_buffers() {
			for (void* q : p) { alpgpu_free(context(), q); }
		}
		void* get(size_t bytes) {
			void* q = nullptr;
			check(alpgpu_malloc(context(), &q, bytes ? bytes : 1), "alpgpu_malloc");
			p.push_back(q);
			return q;
		}
	};
	// A serialized column uploaded whole for the calls that read it where it lies (take, select_range): buffers sized by the blob's header and freed
	// with the object — also when the upload throws (a blob alpgpu_column_from_blob* refuses, an allocation that fails): `buf` is complete by then.
	// alpgpu_column_from_blob* checks the header and every descriptor against the buffers before it copies anything.
	struct uploaded_column {
		device_buffers buf;
		alpgpu_column  col {};
		uint64_t       n_values = 0;
		uploaded_column(const uint8_t* blob, size_t size, const std::string& who) {
			if (size < sizeof(alpgpu_blob_header)) { throw std::runtime_error(who + ": blob shorter than its header"); }
			alpgpu_blob_header h;
			std::memcpy(&h, blob, sizeof(h));
			if (h.n_vectors > (uint64_t(1) << 40) || h.packed_bytes > (uint64_t(1) << 50) || h.exc_bytes > (uint64_t(1) << 50) ||
			    alpgpu_blob_size(h.n_vectors, h.packed_bytes, h.exc_bytes) > size) { // (nothing is allocated beyond what the blob itself holds)
				throw std::runtime_error(who + ": blob header is implausible");
			}
			col.n_vectors       = h.n_vectors;
			col.n_rowgroups     = (h.n_vectors + config::N_VECTORS_PER_ROWGROUP - 1) / config::N_VECTORS_PER_ROWGROUP;
			col.d_rowgroups     = static_cast<alpgpu_rowgroup_state*>(get(col.n_rowgroups * sizeof(alpgpu_rowgroup_state)));
			col.d_vectors       = static_cast<alpgpu_vector_desc*>(get(col.n_vectors * sizeof(alpgpu_vector_desc)));
			col.packed_capacity = h.packed_bytes;
			col.d_packed        = static_cast<uint8_t*>(get(h.packed_bytes));
			col.exc_capacity    = h.exc_bytes;
			col.d_exc           = static_cast<uint8_t*>(get(h.exc_bytes));
			col.d_totals        = static_cast<uint64_t*>(get(8 * sizeof(uint64_t)));
			check(sizeof(PT) == 8 ? alpgpu_column_from_blob(context(), blob, size, &col, &n_values) : alpgpu_column_from_blob_f32(context(), blob, size, &col, &n_values),
			      "alpgpu_column_from_blob");
		}
		void* get(size_t bytes) { return buf.get(bytes); }
	};
	// The n values at value indices idx[0 .. n) of a serialized column (include/alpgpu.h: alpgpu_gather_*): the blob goes up whole (validated by
	// alpgpu_column_from_blob*), the values are gathered where they lie and only they come back.  An index at or past n_vectors * 1024 gives the
	// canonical quiet NaN.
	static std::vector<PT> take(const uint8_t* blob, size_t size, const uint64_t* idx, size_t n) {
		uploaded_column up(blob, size, "alp::gpu::column::take");
		std::vector<PT> out(n);
		if (n == 0) { return out; }
		int64_t* d_idx = static_cast<int64_t*>(up.get(n * sizeof(int64_t)));
		PT*      d_out = static_cast<PT*>(up.get(n * sizeof(PT)));
		check(alpgpu_memcpy_h2d(context(), d_idx, idx, n * sizeof(int64_t)), "alpgpu_memcpy_h2d"); // (an index >= 2^63 reads as negative: out of range either way)
		check(sizeof(PT) == 8 ? alpgpu_gather_f64(context(), &up.col, d_idx, n, reinterpret_cast<double*>(d_out)) : alpgpu_gather_f32(context(), &up.col, d_idx, n, reinterpret_cast<float*>(d_out)),
		      "alpgpu_gather");
		check(alpgpu_memcpy_d2h(context(), out.data(), d_out, n * sizeof(PT)), "alpgpu_memcpy_d2h");
		return out;
	}
	// The values x of a serialized column with lo <= x <= hi and their value indices, ascending (include/alpgpu.h: alpgpu_select_range_*): the blob
	// goes up whole, the predicate is evaluated on the compressed column over [0, n_values) — the tail padding of the last vector never qualifies —
	// and only the selected indices and values come back.  NaN never qualifies; lo > hi selects nothing.
	struct selection {
		std::vector<uint64_t> indices;
		std::vector<PT>       values;
	};
	static selection select_range(const uint8_t* blob, size_t size, PT lo, PT hi) { return select_range_with(blob, size, lo, hi, nullptr); }
	// One record per vector of a column (include/alpgpu.h, "zone maps"): min / max of the vector's values that are not NaN, -0.0 below +0.0,
	// {+inf, -inf} when there is none.  A caller who persists a blob keeps its records beside it and hands them to select_range.
	using zone = typename std::conditional<sizeof(PT) == 8, alpgpu_zone_f64, alpgpu_zone_f32>::type;
	static std::vector<zone> zone_map(const uint8_t* blob, size_t size) {
		uploaded_column   up(blob, size, "alp::gpu::column::zone_map");
		std::vector<zone> out(up.col.n_vectors);
		if (out.empty()) { return out; }
		zone* d_zones = static_cast<zone*>(up.get(out.size() * sizeof(zone)));
		make_zone_map(up, d_zones);
		check(alpgpu_memcpy_d2h(context(), out.data(), d_zones, out.size() * sizeof(zone)), "alpgpu_memcpy_d2h");
		return out;
	}
	// The column's {min, max} (alpgpu_zones_minmax_*): {+inf, -inf} for an empty column or one of NaNs only.
	static zone min_max(const uint8_t* blob, size_t size) {
		uploaded_column up(blob, size, "alp::gpu::column::min_max");
		zone*           d_zones = static_cast<zone*>(up.get(up.col.n_vectors * sizeof(zone)));
		PT*             d_mm    = static_cast<PT*>(up.get(2 * sizeof(PT)));
		make_zone_map(up, d_zones);
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_zones_minmax_f64(context(), d_zones, up.col.n_vectors, reinterpret_cast<double*>(d_mm)), "alpgpu_zones_minmax_f64");
		} else {
			check(alpgpu_zones_minmax_f32(context(), d_zones, up.col.n_vectors, reinterpret_cast<float*>(d_mm)), "alpgpu_zones_minmax_f32");
		}
		zone out;
		check(alpgpu_memcpy_d2h(context(), &out, d_mm, sizeof(out)), "alpgpu_memcpy_d2h");
		return out;
	}
	// select_range with the column's zone map (one record per vector, e.g. zone_map() of the same blob): the same selection; vectors whose
	// record misses [lo, hi] are not decoded (alpgpu_select_range_zoned_*).  Records must contain their vectors' values.
	static selection select_range(const uint8_t* blob, size_t size, PT lo, PT hi, const std::vector<zone>& zones) {
		if (size >= sizeof(alpgpu_blob_header)) {
			alpgpu_blob_header h;
			std::memcpy(&h, blob, sizeof(h));
			if (zones.size() != h.n_vectors) { throw std::runtime_error("alp::gpu::column::select_range: the zone map must hold one record per vector"); }
		}
		return select_range_with(blob, size, lo, hi, &zones);
	}
	// Selection bitmaps (include/alpgpu.h, "selection bitmaps"): the qualify mask of lo <= x <= hi over [0, n_values) as 16 words per vector, bit
	// r & 63 of word r >> 6 = value index r.  Predicates on columns of equal length combine in one mask (mask_and: the bits of tail padding
	// clear; mask_or), mask_indices lists what is left, sum_masked sums another column under it and take_masked projects one.
	enum mask_op { mask_set = ALPGPU_MASK_SET, mask_and = ALPGPU_MASK_AND, mask_or = ALPGPU_MASK_OR };
	static std::vector<uint64_t> select_mask(const uint8_t* blob, size_t size, PT lo, PT hi) {
		std::vector<uint64_t> mask;
		select_mask_with(blob, size, lo, hi, mask_set, mask, true);
		return mask;
	}
	static void select_mask(const uint8_t* blob, size_t size, PT lo, PT hi, mask_op op, std::vector<uint64_t>& mask) { select_mask_with(blob, size, lo, hi, op, mask, false); }
	// the set bits as ascending value indices (alpgpu_mask_to_indices)
	static std::vector<int64_t> mask_indices(const std::vector<uint64_t>& mask) {
		if (mask.size() % 16 != 0) { throw std::runtime_error("alp::gpu::column::mask_indices: a mask holds 16 words per vector"); }
		std::vector<int64_t> out;
		const uint64_t       n_vectors = mask.size() / 16;
		if (n_vectors == 0) { return out; }
		device_buffers buf;
		uint64_t*      d_mask    = static_cast<uint64_t*>(buf.get(mask.size() * sizeof(uint64_t)));
		uint64_t*      d_count   = static_cast<uint64_t*>(buf.get(sizeof(uint64_t)));
		void*          d_scratch = buf.get(alpgpu_select_scratch_bytes(n_vectors));
		check(alpgpu_memcpy_h2d(context(), d_mask, mask.data(), mask.size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d");
		uint64_t count = 0;
		check(alpgpu_mask_to_indices(context(), d_mask, n_vectors, nullptr, 0, d_count, d_scratch), "alpgpu_mask_to_indices"); // count first, then allocate exactly
		check(alpgpu_memcpy_d2h(context(), &count, d_count, sizeof(count)), "alpgpu_memcpy_d2h");
		if (count == 0) { return out; }
		int64_t* d_idx = static_cast<int64_t*>(buf.get(count * sizeof(int64_t)));
		check(alpgpu_mask_to_indices(context(), d_mask, n_vectors, d_idx, count, d_count, d_scratch), "alpgpu_mask_to_indices");
		out.resize(count);
		check(alpgpu_memcpy_d2h(context(), out.data(), d_idx, count * sizeof(int64_t)), "alpgpu_memcpy_d2h");
		return out;
	}
	// SUM and COUNT of the column's values whose bit is set (alpgpu_decode_sum_masked_* and alpgpu_tree_sum_f64 over its per-vector sums: the
	// order include/alpgpu.h documents, so the same blob and mask give the same bits every time)
	struct masked_sum {
		double   sum;
		uint64_t count;
	};
	static masked_sum sum_masked(const uint8_t* blob, size_t size, const std::vector<uint64_t>& mask) {
		uploaded_column up(blob, size, "alp::gpu::column::sum_masked");
		const uint64_t  nv = up.col.n_vectors;
		if (mask.size() != 16 * nv) { throw std::runtime_error("alp::gpu::column::sum_masked: the mask must hold 16 words per vector"); }
		masked_sum out {0.0, 0};
		if (nv == 0) { return out; }
		uint64_t* d_mask   = static_cast<uint64_t*>(up.get(mask.size() * sizeof(uint64_t)));
		double*   d_sums   = static_cast<double*>(up.get(nv * sizeof(double)));
		uint32_t* d_counts = static_cast<uint32_t*>(up.get(nv * sizeof(uint32_t)));
		double*   d_total  = static_cast<double*>(up.get(sizeof(double)));
		check(alpgpu_memcpy_h2d(context(), d_mask, mask.data(), mask.size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d");
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_decode_sum_masked_f64(context(), &up.col, d_mask, d_sums, d_counts), "alpgpu_decode_sum_masked_f64");
		} else {
			check(alpgpu_decode_sum_masked_f32(context(), &up.col, d_mask, d_sums, d_counts), "alpgpu_decode_sum_masked_f32");
		}
		check(alpgpu_tree_sum_f64(context(), d_sums, nv, d_total), "alpgpu_tree_sum_f64");
		std::vector<uint32_t> counts(nv);
		check(alpgpu_memcpy_d2h(context(), &out.sum, d_total, sizeof(double)), "alpgpu_memcpy_d2h");
		check(alpgpu_memcpy_d2h(context(), counts.data(), d_counts, nv * sizeof(uint32_t)), "alpgpu_memcpy_d2h");
		for (uint32_t c : counts) { out.count += c; }
		return out;
	}
	// Two-column consumers (include/alpgpu.h, "two-column consumers"): this column (blob a) against another serialized column of the same type and
	// the same number of values (blob b; the same blob is allowed).  compare_mask: the qualify mask of a_r CMP b_r over [0, n_values) with C's
	// comparison (a NaN on either side: only cmp_ne holds), fresh or combined into a mask as select_mask combines; the bits of tail padding
	// come out clear under mask_set and mask_and.
	enum compare_op { cmp_lt = ALPGPU_CMP_LT, cmp_le = ALPGPU_CMP_LE, cmp_gt = ALPGPU_CMP_GT, cmp_ge = ALPGPU_CMP_GE, cmp_eq = ALPGPU_CMP_EQ, cmp_ne = ALPGPU_CMP_NE };
	static std::vector<uint64_t> compare_mask(const uint8_t* blob_a, size_t size_a, const uint8_t* blob_b, size_t size_b, compare_op cmp) {
		std::vector<uint64_t> mask;
		compare_mask_with(blob_a, size_a, blob_b, size_b, cmp, mask_set, mask, true);
		return mask;
	}
	static void compare_mask(const uint8_t* blob_a, size_t size_a, const uint8_t* blob_b, size_t size_b, compare_op cmp, mask_op op, std::vector<uint64_t>& mask) {
		compare_mask_with(blob_a, size_a, blob_b, size_b, cmp, op, mask, false);
	}
	// SUM(a * b) and COUNT over the set bits (alpgpu_decode_dot_masked_* and alpgpu_tree_sum_f64 over its per-vector sums: product and sum rounded
	// separately in the order include/alpgpu.h documents, so the same blobs and mask give the same bits every time)
	static masked_sum dot_masked(const uint8_t* blob_a, size_t size_a, const uint8_t* blob_b, size_t size_b, const std::vector<uint64_t>& mask) {
		uploaded_column a(blob_a, size_a, "alp::gpu::column::dot_masked"), b(blob_b, size_b, "alp::gpu::column::dot_masked");
		const uint64_t  nv = a.col.n_vectors;
		if (b.col.n_vectors != nv) { throw std::runtime_error("alp::gpu::column::dot_masked: the columns differ in length"); }
		if (mask.size() != 16 * nv) { throw std::runtime_error("alp::gpu::column::dot_masked: the mask must hold 16 words per vector"); }
		masked_sum out {0.0, 0};
		if (nv == 0) { return out; }
		uint64_t* d_mask   = static_cast<uint64_t*>(a.get(mask.size() * sizeof(uint64_t)));
		double*   d_sums   = static_cast<double*>(a.get(nv * sizeof(double)));
		uint32_t* d_counts = static_cast<uint32_t*>(a.get(nv * sizeof(uint32_t)));
		double*   d_total  = static_cast<double*>(a.get(sizeof(double)));
		check(alpgpu_memcpy_h2d(context(), d_mask, mask.data(), mask.size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d");
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_decode_dot_masked_f64(context(), &a.col, &b.col, d_mask, d_sums, d_counts), "alpgpu_decode_dot_masked_f64");
		} else {
			check(alpgpu_decode_dot_masked_f32(context(), &a.col, &b.col, d_mask, d_sums, d_counts), "alpgpu_decode_dot_masked_f32");
		}
		check(alpgpu_tree_sum_f64(context(), d_sums, nv, d_total), "alpgpu_tree_sum_f64");
		std::vector<uint32_t> counts(nv);
		check(alpgpu_memcpy_d2h(context(), &out.sum, d_total, sizeof(double)), "alpgpu_memcpy_d2h");
		check(alpgpu_memcpy_d2h(context(), counts.data(), d_counts, nv * sizeof(uint32_t)), "alpgpu_memcpy_d2h");
		for (uint32_t c : counts) { out.count += c; }
		return out;
	}
	// Grouped aggregation (include/alpgpu.h, "grouped aggregation"): this column (blob val) summed and counted per vector, under the mask, for the
	// n_groups closed ranges lo[g] <= k <= hi[g] of a key column of the same type and length (blob key; the same blob is allowed), all in one pass
	// over the two columns (alpgpu_decode_group_sum_*).  sums and counts (optional) come back as [n_groups][n_vectors], row g bit for bit what
	// sum_masked's per-vector pass gives under the mask ANDed with select_mask(key, lo[g], hi[g]).  Returns n_vectors.
	static uint64_t group_sum_masked(const uint8_t* blob_val, size_t size_val, const uint8_t* blob_key, size_t size_key, const std::vector<uint64_t>& mask, const PT* lo, const PT* hi,
	                                 uint32_t n_groups, std::vector<double>& sums, std::vector<uint32_t>* counts = nullptr) {
		if (n_groups == 0 || n_groups > ALPGPU_GROUP_MAX || !lo || !hi) { throw std::runtime_error("alp::gpu::column::group_sum_masked: 1 .. ALPGPU_GROUP_MAX groups with their bounds"); }
		uploaded_column val(blob_val, size_val, "alp::gpu::column::group_sum_masked"), key(blob_key, size_key, "alp::gpu::column::group_sum_masked");
		const uint64_t  nv = val.col.n_vectors;
		if (key.col.n_vectors != nv) { throw std::runtime_error("alp::gpu::column::group_sum_masked: the columns differ in length"); }
		if (mask.size() != 16 * nv) { throw std::runtime_error("alp::gpu::column::group_sum_masked: the mask must hold 16 words per vector"); }
		sums.assign(n_groups * nv, 0.0);
		if (counts) { counts->assign(n_groups * nv, 0); }
		if (nv == 0) { return nv; }
		uint64_t* d_mask   = static_cast<uint64_t*>(val.get(mask.size() * sizeof(uint64_t)));
		double*   d_sums   = static_cast<double*>(val.get(sums.size() * sizeof(double)));
		uint32_t* d_counts = counts ? static_cast<uint32_t*>(val.get(sums.size() * sizeof(uint32_t))) : nullptr;
		check(alpgpu_memcpy_h2d(context(), d_mask, mask.data(), mask.size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d");
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_decode_group_sum_f64(context(), &val.col, &key.col, d_mask, lo, hi, n_groups, d_sums, d_counts), "alpgpu_decode_group_sum_f64");
		} else {
			check(alpgpu_decode_group_sum_f32(context(), &val.col, &key.col, d_mask, lo, hi, n_groups, d_sums, d_counts), "alpgpu_decode_group_sum_f32");
		}
		check(alpgpu_memcpy_d2h(context(), sums.data(), d_sums, sums.size() * sizeof(double)), "alpgpu_memcpy_d2h");
		if (counts) { check(alpgpu_memcpy_d2h(context(), counts->data(), d_counts, counts->size() * sizeof(uint32_t)), "alpgpu_memcpy_d2h"); }
		return nv;
	}
	// Every group's SUM and COUNT from what group_sum_masked returned (alpgpu_group_totals: each row by the tree of alpgpu_tree_sum_f64, the counts
	// added exactly; without counts every count is 0)
	static std::vector<masked_sum> group_totals(const std::vector<double>& sums, const std::vector<uint32_t>* counts, uint64_t n_vectors, uint32_t n_groups) {
		if (n_groups == 0 || n_groups > ALPGPU_GROUP_MAX || sums.size() != n_groups * n_vectors || (counts && counts->size() != sums.size())) {
			throw std::runtime_error("alp::gpu::column::group_totals: sums (and counts) must be [n_groups][n_vectors], 1 .. ALPGPU_GROUP_MAX groups");
		}
		device_buffers buf;
		double*        d_sums    = static_cast<double*>(buf.get(sums.size() * sizeof(double)));
		uint32_t*      d_counts  = counts ? static_cast<uint32_t*>(buf.get(sums.size() * sizeof(uint32_t))) : nullptr;
		double*        d_totals  = static_cast<double*>(buf.get(n_groups * sizeof(double)));
		uint64_t*      d_tcounts = counts ? static_cast<uint64_t*>(buf.get(n_groups * sizeof(uint64_t))) : nullptr;
		void*          d_scratch = buf.get(alpgpu_group_totals_scratch_bytes(n_vectors, n_groups));
		if (!sums.empty()) { check(alpgpu_memcpy_h2d(context(), d_sums, sums.data(), sums.size() * sizeof(double)), "alpgpu_memcpy_h2d"); }
		if (counts && !sums.empty()) { check(alpgpu_memcpy_h2d(context(), d_counts, counts->data(), sums.size() * sizeof(uint32_t)), "alpgpu_memcpy_h2d"); }
		check(alpgpu_group_totals(context(), d_sums, d_counts, n_vectors, n_groups, d_totals, d_tcounts, d_scratch), "alpgpu_group_totals");
		std::vector<double>   totals(n_groups);
		std::vector<uint64_t> tcounts(n_groups, 0);
		check(alpgpu_memcpy_d2h(context(), totals.data(), d_totals, n_groups * sizeof(double)), "alpgpu_memcpy_d2h");
		if (counts) { check(alpgpu_memcpy_d2h(context(), tcounts.data(), d_tcounts, n_groups * sizeof(uint64_t)), "alpgpu_memcpy_d2h"); }
		std::vector<masked_sum> out(n_groups);
		for (uint32_t g = 0; g < n_groups; ++g) { out[g] = masked_sum {totals[g], tcounts[g]}; }
		return out;
	}
	// Masked and grouped MIN / MAX (include/alpgpu.h, "masked and grouped MIN / MAX").  minmax_masked: one record per vector over the values whose
	// bit is set (alpgpu_decode_minmax_masked_*), with the rules of zone_map — NaNs ignored, -0.0 below +0.0, {+inf, -inf} when nothing selected is
	// a number — and, optionally, each vector's number of set bits.  The records are narrower than the vectors' intervals: not for select_range.
	static std::vector<zone> minmax_masked(const uint8_t* blob, size_t size, const std::vector<uint64_t>& mask, std::vector<uint32_t>* counts = nullptr) {
		uploaded_column up(blob, size, "alp::gpu::column::minmax_masked");
		const uint64_t  nv = up.col.n_vectors;
		if (mask.size() != 16 * nv) { throw std::runtime_error("alp::gpu::column::minmax_masked: the mask must hold 16 words per vector"); }
		std::vector<zone> out(nv);
		if (counts) { counts->assign(nv, 0); }
		if (nv == 0) { return out; }
		uint64_t* d_mask   = static_cast<uint64_t*>(up.get(mask.size() * sizeof(uint64_t)));
		zone*     d_zones  = static_cast<zone*>(up.get(nv * sizeof(zone)));
		uint32_t* d_counts = counts ? static_cast<uint32_t*>(up.get(nv * sizeof(uint32_t))) : nullptr;
		check(alpgpu_memcpy_h2d(context(), d_mask, mask.data(), mask.size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d");
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_decode_minmax_masked_f64(context(), &up.col, d_mask, d_zones, d_counts), "alpgpu_decode_minmax_masked_f64");
		} else {
			check(alpgpu_decode_minmax_masked_f32(context(), &up.col, d_mask, d_zones, d_counts), "alpgpu_decode_minmax_masked_f32");
		}
		check(alpgpu_memcpy_d2h(context(), out.data(), d_zones, nv * sizeof(zone)), "alpgpu_memcpy_d2h");
		if (counts) { check(alpgpu_memcpy_d2h(context(), counts->data(), d_counts, nv * sizeof(uint32_t)), "alpgpu_memcpy_d2h"); }
		return out;
	}
	// Top-k (include/alpgpu.h, "top-k"): ORDER BY x [DESC] LIMIT k over the values whose bit is set (alpgpu_top_k_*).  values[j], indices[j] are the
	// j-th element, the largest (largest = false: the smallest) first; NaNs are left out, -0.0 lies below +0.0, equal bit patterns come by ascending
	// index, and each value has the bits decompress gives it.  Both vectors are min(k, selected values that are no NaNs) long; k <= ALPGPU_TOP_K_MAX.
	// records (optional): the EXACT masked records of this column under this mask, as minmax_masked returns them — the call then skips its first
	// decode pass; any other records give an unspecified selection.
	struct top_k_result {
		std::vector<PT>      values;
		std::vector<int64_t> indices;
	};
	static top_k_result top_k(const uint8_t* blob, size_t size, const std::vector<uint64_t>& mask, uint64_t k, bool largest = true, const std::vector<zone>* records = nullptr) {
		uploaded_column up(blob, size, "alp::gpu::column::top_k");
		const uint64_t  nv = up.col.n_vectors;
		if (mask.size() != 16 * nv) { throw std::runtime_error("alp::gpu::column::top_k: the mask must hold 16 words per vector"); }
		if (k > ALPGPU_TOP_K_MAX) { throw std::runtime_error("alp::gpu::column::top_k: k must not be more than ALPGPU_TOP_K_MAX"); }
		if (records && records->size() != nv) { throw std::runtime_error("alp::gpu::column::top_k: one record per vector"); }
		top_k_result out;
		if (nv == 0 || k == 0) { return out; }
		uint64_t* d_mask    = static_cast<uint64_t*>(up.get(mask.size() * sizeof(uint64_t)));
		zone*     d_records = records ? static_cast<zone*>(up.get(nv * sizeof(zone))) : nullptr;
		PT*       d_vals    = static_cast<PT*>(up.get(k * sizeof(PT)));
		int64_t*  d_idx     = static_cast<int64_t*>(up.get(k * sizeof(int64_t)));
		uint64_t* d_count   = static_cast<uint64_t*>(up.get(sizeof(uint64_t)));
		void*     d_scratch = up.get(alpgpu_top_k_scratch_bytes(nv, k));
		check(alpgpu_memcpy_h2d(context(), d_mask, mask.data(), mask.size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d");
		if (records) { check(alpgpu_memcpy_h2d(context(), d_records, records->data(), nv * sizeof(zone)), "alpgpu_memcpy_h2d"); }
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_top_k_f64(context(), &up.col, d_mask, d_records, k, largest ? 1 : 0, reinterpret_cast<double*>(d_vals), d_idx, d_count, d_scratch), "alpgpu_top_k_f64");
		} else {
			check(alpgpu_top_k_f32(context(), &up.col, d_mask, d_records, k, largest ? 1 : 0, reinterpret_cast<float*>(d_vals), d_idx, d_count, d_scratch), "alpgpu_top_k_f32");
		}
		uint64_t count = 0;
		check(alpgpu_memcpy_d2h(context(), &count, d_count, sizeof(count)), "alpgpu_memcpy_d2h");
		if (count > k) { throw std::runtime_error("alp::gpu::column::top_k: the count exceeds k"); }
		out.values.resize(count);
		out.indices.resize(count);
		if (count > 0) {
			check(alpgpu_memcpy_d2h(context(), out.values.data(), d_vals, count * sizeof(PT)), "alpgpu_memcpy_d2h");
			check(alpgpu_memcpy_d2h(context(), out.indices.data(), d_idx, count * sizeof(int64_t)), "alpgpu_memcpy_d2h");
		}
		return out;
	}
	// Quantiles (include/alpgpu.h, "quantiles"): order statistics over the values whose bit is set and that are no NaNs, N = count of them, in the
	// order of top_k (-0.0 below +0.0); every value has the bits decompress gives it.  select_rank: lower[i] = the min(ranks[i], N - 1)-th smallest
	// (from_top: largest), 1 .. ALPGPU_RANK_MAX ranks in any order; upper and ranks stay empty.  quantile: for each q[i] in [0, 1] (1 ..
	// ALPGPU_QUANTILE_MAX) ranks[i] = min(N - 1, floor(q[i] * (N - 1))), lower[i] the value at that rank and upper[i] the one at the next (the
	// last: itself), what PERCENTILE_DISC and, interpolated by the caller, PERCENTILE_CONT need.  With count == 0 the vectors are empty.
	// zones (optional): any records that contain the vectors' masked intervals (zone_map, minmax_masked, widened ones); they change no value.
	struct quantile_result {
		std::vector<PT>       lower, upper;
		std::vector<uint64_t> ranks;
		uint64_t              count = 0;
	};
	static quantile_result select_rank(const uint8_t* blob, size_t size, const std::vector<uint64_t>& mask, const std::vector<uint64_t>& ranks, bool from_top = false,
	                                   const std::vector<zone>* zones = nullptr) {
		if (ranks.empty() || ranks.size() > ALPGPU_RANK_MAX) { throw std::runtime_error("alp::gpu::column::select_rank: 1 .. ALPGPU_RANK_MAX ranks"); }
		return order_statistics(blob, size, mask, ranks.data(), nullptr, static_cast<uint32_t>(ranks.size()), from_top, zones, "alp::gpu::column::select_rank");
	}
	static quantile_result quantile(const uint8_t* blob, size_t size, const std::vector<uint64_t>& mask, const std::vector<double>& q, const std::vector<zone>* zones = nullptr) {
		if (q.empty() || q.size() > ALPGPU_QUANTILE_MAX) { throw std::runtime_error("alp::gpu::column::quantile: 1 .. ALPGPU_QUANTILE_MAX quantiles"); }
		for (const double x : q) {
			if (!(x >= 0.0 && x <= 1.0)) { throw std::runtime_error("alp::gpu::column::quantile: a quantile lies outside [0, 1]"); }
		}
		return order_statistics(blob, size, mask, nullptr, q.data(), static_cast<uint32_t>(q.size()), false, zones, "alp::gpu::column::quantile");
	}

  private:
	static quantile_result order_statistics(const uint8_t* blob, size_t size, const std::vector<uint64_t>& mask, const uint64_t* ranks, const double* q, uint32_t n, bool from_top,
	                                        const std::vector<zone>* zones, const char* who) {
		uploaded_column up(blob, size, who);
		const uint64_t  nv = up.col.n_vectors;
		if (mask.size() != 16 * nv) { throw std::runtime_error(std::string(who) + ": the mask must hold 16 words per vector"); }
		if (zones && zones->size() != nv) { throw std::runtime_error(std::string(who) + ": one record per vector"); }
		quantile_result out;
		if (nv == 0) { return out; }
		const uint32_t n_vals   = q ? 2 * n : n;
		uint64_t*      d_mask   = static_cast<uint64_t*>(up.get(mask.size() * sizeof(uint64_t)));
		zone*          d_zones  = zones ? static_cast<zone*>(up.get(nv * sizeof(zone))) : nullptr;
		PT*            d_vals   = static_cast<PT*>(up.get(n_vals * sizeof(PT)));
		uint64_t*      d_ranks  = static_cast<uint64_t*>(up.get(n * sizeof(uint64_t)));
		uint64_t*      d_count  = static_cast<uint64_t*>(up.get(sizeof(uint64_t)));
		void*          d_scratch = up.get(alpgpu_quantile_scratch_bytes(nv));
		check(alpgpu_memcpy_h2d(context(), d_mask, mask.data(), mask.size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d");
		if (zones) { check(alpgpu_memcpy_h2d(context(), d_zones, zones->data(), nv * sizeof(zone)), "alpgpu_memcpy_h2d"); }
		if constexpr (sizeof(PT) == 8) {
			if (q) {
				check(alpgpu_quantile_f64(context(), &up.col, d_mask, d_zones, q, n, reinterpret_cast<double*>(d_vals), d_ranks, d_count, d_scratch), "alpgpu_quantile_f64");
			} else {
				check(alpgpu_select_rank_f64(context(), &up.col, d_mask, d_zones, ranks, n, from_top ? 1 : 0, reinterpret_cast<double*>(d_vals), d_count, d_scratch), "alpgpu_select_rank_f64");
			}
		} else {
			if (q) {
				check(alpgpu_quantile_f32(context(), &up.col, d_mask, d_zones, q, n, reinterpret_cast<float*>(d_vals), d_ranks, d_count, d_scratch), "alpgpu_quantile_f32");
			} else {
				check(alpgpu_select_rank_f32(context(), &up.col, d_mask, d_zones, ranks, n, from_top ? 1 : 0, reinterpret_cast<float*>(d_vals), d_count, d_scratch), "alpgpu_select_rank_f32");
			}
		}
		check(alpgpu_memcpy_d2h(context(), &out.count, d_count, sizeof(out.count)), "alpgpu_memcpy_d2h");
		if (out.count == 0) { return out; }
		std::vector<PT> vals(n_vals);
		check(alpgpu_memcpy_d2h(context(), vals.data(), d_vals, n_vals * sizeof(PT)), "alpgpu_memcpy_d2h");
		if (q) {
			out.ranks.resize(n);
			check(alpgpu_memcpy_d2h(context(), out.ranks.data(), d_ranks, n * sizeof(uint64_t)), "alpgpu_memcpy_d2h");
			for (uint32_t i = 0; i < n; ++i) {
				out.lower.push_back(vals[2 * i]);
				out.upper.push_back(vals[2 * i + 1]);
			}
		} else {
			out.lower = vals;
		}
		return out;
	}

  public:
	// group_minmax_masked: group_sum_masked's arguments; zones and counts (optional) come back as [n_groups][n_vectors], row g bit for bit what
	// minmax_masked gives under the mask ANDed with select_mask(key, lo[g], hi[g]) (alpgpu_decode_group_minmax_*).  Returns n_vectors.
	static uint64_t group_minmax_masked(const uint8_t* blob_val, size_t size_val, const uint8_t* blob_key, size_t size_key, const std::vector<uint64_t>& mask, const PT* lo, const PT* hi,
	                                    uint32_t n_groups, std::vector<zone>& zones, std::vector<uint32_t>* counts = nullptr) {
		if (n_groups == 0 || n_groups > ALPGPU_GROUP_MAX || !lo || !hi) { throw std::runtime_error("alp::gpu::column::group_minmax_masked: 1 .. ALPGPU_GROUP_MAX groups with their bounds"); }
		uploaded_column val(blob_val, size_val, "alp::gpu::column::group_minmax_masked"), key(blob_key, size_key, "alp::gpu::column::group_minmax_masked");
		const uint64_t  nv = val.col.n_vectors;
		if (key.col.n_vectors != nv) { throw std::runtime_error("alp::gpu::column::group_minmax_masked: the columns differ in length"); }
		if (mask.size() != 16 * nv) { throw std::runtime_error("alp::gpu::column::group_minmax_masked: the mask must hold 16 words per vector"); }
		zones.assign(n_groups * nv, zone {});
		if (counts) { counts->assign(n_groups * nv, 0); }
		if (nv == 0) { return nv; }
		uint64_t* d_mask   = static_cast<uint64_t*>(val.get(mask.size() * sizeof(uint64_t)));
		zone*     d_zones  = static_cast<zone*>(val.get(zones.size() * sizeof(zone)));
		uint32_t* d_counts = counts ? static_cast<uint32_t*>(val.get(zones.size() * sizeof(uint32_t))) : nullptr;
		check(alpgpu_memcpy_h2d(context(), d_mask, mask.data(), mask.size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d");
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_decode_group_minmax_f64(context(), &val.col, &key.col, d_mask, lo, hi, n_groups, d_zones, d_counts), "alpgpu_decode_group_minmax_f64");
		} else {
			check(alpgpu_decode_group_minmax_f32(context(), &val.col, &key.col, d_mask, lo, hi, n_groups, d_zones, d_counts), "alpgpu_decode_group_minmax_f32");
		}
		check(alpgpu_memcpy_d2h(context(), zones.data(), d_zones, zones.size() * sizeof(zone)), "alpgpu_memcpy_d2h");
		if (counts) { check(alpgpu_memcpy_d2h(context(), counts->data(), d_counts, counts->size() * sizeof(uint32_t)), "alpgpu_memcpy_d2h"); }
		return nv;
	}
	// Every group's {min, max} from what group_minmax_masked returned (alpgpu_group_minmax_totals_*); {+inf, -inf} for n_vectors == 0
	static std::vector<zone> group_minmax_totals(const std::vector<zone>& zones, uint64_t n_vectors, uint32_t n_groups) {
		if (n_groups == 0 || n_groups > ALPGPU_GROUP_MAX || zones.size() != n_groups * n_vectors) {
			throw std::runtime_error("alp::gpu::column::group_minmax_totals: zones must be [n_groups][n_vectors], 1 .. ALPGPU_GROUP_MAX groups");
		}
		device_buffers buf;
		zone*          d_zones  = static_cast<zone*>(buf.get(zones.size() * sizeof(zone)));
		zone*          d_totals = static_cast<zone*>(buf.get(n_groups * sizeof(zone)));
		if (!zones.empty()) { check(alpgpu_memcpy_h2d(context(), d_zones, zones.data(), zones.size() * sizeof(zone)), "alpgpu_memcpy_h2d"); }
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_group_minmax_totals_f64(context(), d_zones, n_vectors, n_groups, reinterpret_cast<double*>(d_totals)), "alpgpu_group_minmax_totals_f64");
		} else {
			check(alpgpu_group_minmax_totals_f32(context(), d_zones, n_vectors, n_groups, reinterpret_cast<float*>(d_totals)), "alpgpu_group_minmax_totals_f32");
		}
		std::vector<zone> out(n_groups);
		check(alpgpu_memcpy_d2h(context(), out.data(), d_totals, n_groups * sizeof(zone)), "alpgpu_memcpy_d2h");
		return out;
	}
	// Set membership (include/alpgpu.h, "set membership"): the mask of `x IN (values)` over [0, n_values) — with negate, of `x NOT IN (values)`, which a
	// NaN value satisfies — fresh, or combined into a mask as select_mask combines.  member(x): some element == x (-0.0 == 0.0, a NaN never).  The
	// values are sorted here, on the host (NaNs last, nothing dropped), as alpgpu_select_in_mask_* wants its list.
	static std::vector<uint64_t> select_in_mask(const uint8_t* blob, size_t size, const std::vector<PT>& values, bool negate = false) {
		std::vector<uint64_t> mask;
		select_in_mask_with(blob, size, values, negate, mask_set, mask, true);
		return mask;
	}
	static void select_in_mask(const uint8_t* blob, size_t size, const std::vector<PT>& values, bool negate, mask_op op, std::vector<uint64_t>& mask) {
		select_in_mask_with(blob, size, values, negate, op, mask, false);
	}
	// Histograms (include/alpgpu.h, "histograms"): the bucket counts of the values [0, n_values) whose bit is set in the mask (nullptr: all of them) by
	// the edges, edges.size() + 2 words: word b counts the values with b edges <= x (right: < x), so word 0 lies below the first edge and word
	// edges.size() at or above the last; the last word counts the NaNs.  -0.0 == 0.0, +-inf are ordinary.  The edges (at most
	// ALPGPU_HISTOGRAM_EDGES_MAX) are sorted here, on the host (NaNs last, where they are inert; duplicates give empty buckets).  zones (optional): any
	// records that contain the vectors' intervals; they change no count.
	static std::vector<uint64_t> histogram(const uint8_t* blob, size_t size, const std::vector<PT>& edges, bool right = false, const std::vector<uint64_t>* mask = nullptr,
	                                       const std::vector<zone>* zones = nullptr) {
		if (edges.size() > ALPGPU_HISTOGRAM_EDGES_MAX) { throw std::runtime_error("alp::gpu::column::histogram: at most ALPGPU_HISTOGRAM_EDGES_MAX edges"); }
		uploaded_column up(blob, size, "alp::gpu::column::histogram");
		const uint64_t  nv = up.col.n_vectors;
		if (mask && mask->size() != 16 * nv) { throw std::runtime_error("alp::gpu::column::histogram: the mask must hold 16 words per vector"); }
		if (zones && zones->size() != nv) { throw std::runtime_error("alp::gpu::column::histogram: one record per vector"); }
		std::vector<uint64_t> counts(edges.size() + 2, 0);
		if (nv == 0) { return counts; }
		std::vector<PT> list(edges);
		std::sort(list.begin(), list.end(), [](PT a, PT b) { return b != b ? a == a : a < b; }); // ascending by <, NaNs last
		uint64_t* d_mask   = mask ? static_cast<uint64_t*>(up.get(mask->size() * sizeof(uint64_t))) : nullptr;
		zone*     d_zones  = zones ? static_cast<zone*>(up.get(nv * sizeof(zone))) : nullptr;
		PT*       d_edges  = list.empty() ? nullptr : static_cast<PT*>(up.get(list.size() * sizeof(PT)));
		uint64_t* d_counts = static_cast<uint64_t*>(up.get(counts.size() * sizeof(uint64_t)));
		if (mask) { check(alpgpu_memcpy_h2d(context(), d_mask, mask->data(), mask->size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d"); }
		if (zones) { check(alpgpu_memcpy_h2d(context(), d_zones, zones->data(), nv * sizeof(zone)), "alpgpu_memcpy_h2d"); }
		if (d_edges) { check(alpgpu_memcpy_h2d(context(), d_edges, list.data(), list.size() * sizeof(PT)), "alpgpu_memcpy_h2d"); }
		const uint32_t n_edges = static_cast<uint32_t>(list.size());
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_histogram_f64(context(), &up.col, 0, up.n_values, d_mask, d_zones, reinterpret_cast<const double*>(d_edges), n_edges, right ? 1 : 0, 0, d_counts), "alpgpu_histogram_f64");
		} else {
			check(alpgpu_histogram_f32(context(), &up.col, 0, up.n_values, d_mask, d_zones, reinterpret_cast<const float*>(d_edges), n_edges, right ? 1 : 0, 0, d_counts), "alpgpu_histogram_f32");
		}
		check(alpgpu_memcpy_d2h(context(), counts.data(), d_counts, counts.size() * sizeof(uint64_t)), "alpgpu_memcpy_d2h");
		return counts;
	}
	// Keyed aggregation (include/alpgpu.h, "keyed aggregation"): SUM and COUNT of this column (blob val) per key of a key column of the same type and
	// length (blob key; the same blob is allowed), over the rows whose bit is set in the mask (nullptr: all of them), in one pass over the two columns
	// (alpgpu_decode_keyed_sum_*).  keys: 1 .. ALPGPU_KEYED_KEYS_MAX keys, sorted here, on the host (NaNs last, where they match nothing); keys, sums
	// and counts come back in that order.  A row belongs to the first key equal to its value of the key column (-0.0 == 0.0); later duplicates get
	// +0.0 and 0; unmatched counts the selected rows without a key.  The sums are in the order include/alpgpu.h documents: the same blobs, mask and
	// keys give the same bits every time.  zones (optional): any records that contain the KEY vectors' intervals; they change no bit.
	struct keyed_result {
		std::vector<PT>       keys;
		std::vector<double>   sums;
		std::vector<uint64_t> counts;
		uint64_t              unmatched = 0;
	};
	static keyed_result sum_by_key(const uint8_t* blob_val, size_t size_val, const uint8_t* blob_key, size_t size_key, const std::vector<uint64_t>* mask, const std::vector<zone>* zones,
	                               const PT* keys, size_t n_keys) {
		static_assert(sizeof(PT) == 8, "alp::gpu::column::sum_by_key is built for double columns only (include/alpgpu.h, \"keyed aggregation\")");
		if (!keys || n_keys == 0 || n_keys > ALPGPU_KEYED_KEYS_MAX) { throw std::runtime_error("alp::gpu::column::sum_by_key: 1 .. ALPGPU_KEYED_KEYS_MAX keys"); }
		uploaded_column val(blob_val, size_val, "alp::gpu::column::sum_by_key"), key(blob_key, size_key, "alp::gpu::column::sum_by_key");
		const uint64_t  nv = val.col.n_vectors;
		if (key.col.n_vectors != nv) { throw std::runtime_error("alp::gpu::column::sum_by_key: the columns differ in length"); }
		if (mask && mask->size() != 16 * nv) { throw std::runtime_error("alp::gpu::column::sum_by_key: the mask must hold 16 words per vector"); }
		if (zones && zones->size() != nv) { throw std::runtime_error("alp::gpu::column::sum_by_key: one record per vector"); }
		keyed_result out;
		out.keys.assign(keys, keys + n_keys);
		std::sort(out.keys.begin(), out.keys.end(), [](PT a, PT b) { return b != b ? a == a : a < b; }); // ascending by <, NaNs last
		out.sums.assign(n_keys, 0.0);
		out.counts.assign(n_keys, 0);
		if (nv == 0) { return out; }
		uint64_t* d_mask    = mask ? static_cast<uint64_t*>(val.get(mask->size() * sizeof(uint64_t))) : nullptr;
		zone*     d_zones   = zones ? static_cast<zone*>(val.get(nv * sizeof(zone))) : nullptr;
		PT*       d_keys    = static_cast<PT*>(val.get(n_keys * sizeof(PT)));
		double*   d_sums    = static_cast<double*>(val.get(n_keys * sizeof(double)));
		uint64_t* d_counts  = static_cast<uint64_t*>(val.get((n_keys + 1) * sizeof(uint64_t)));
		void*     d_scratch = val.get(alpgpu_keyed_sum_scratch_bytes(nv, static_cast<uint32_t>(n_keys)));
		if (mask) { check(alpgpu_memcpy_h2d(context(), d_mask, mask->data(), mask->size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d"); }
		if (zones) { check(alpgpu_memcpy_h2d(context(), d_zones, zones->data(), nv * sizeof(zone)), "alpgpu_memcpy_h2d"); }
		check(alpgpu_memcpy_h2d(context(), d_keys, out.keys.data(), n_keys * sizeof(PT)), "alpgpu_memcpy_h2d");
		check(alpgpu_decode_keyed_sum_f64(context(), &val.col, &key.col, d_mask, reinterpret_cast<const alpgpu_zone_f64*>(d_zones), reinterpret_cast<const double*>(d_keys),
		                                  static_cast<uint32_t>(n_keys), d_sums, d_counts, d_scratch),
		      "alpgpu_decode_keyed_sum_f64");
		std::vector<uint64_t> counts(n_keys + 1);
		check(alpgpu_memcpy_d2h(context(), out.sums.data(), d_sums, n_keys * sizeof(double)), "alpgpu_memcpy_d2h");
		check(alpgpu_memcpy_d2h(context(), counts.data(), d_counts, counts.size() * sizeof(uint64_t)), "alpgpu_memcpy_d2h");
		out.counts.assign(counts.begin(), counts.end() - 1);
		out.unmatched = counts.back();
		return out;
	}
	// Exact keyed SUM (include/alpgpu.h, "exact keyed SUM": alpgpu_decode_keyed_exact_sum_*): sum_by_key's arguments, key handling and result for up
	// to ALPGPU_KEYED_MANY_KEYS_MAX = 2^20 keys and for double AND float columns, every sum the correctly rounded real sum of its rows (a double for
	// both precisions): a NaN if a NaN or both infinities are among them, +-inf where it rounds beyond DBL_MAX, +0.0 for a key without rows.  The sums
	// do not depend on the order of the rows, the grid or the device.  At most ALPGPU_KEYED_EXACT_VECTORS_MAX vectors per column.
	static keyed_result sum_by_key_exact(const uint8_t* blob_val, size_t size_val, const uint8_t* blob_key, size_t size_key, const std::vector<uint64_t>* mask,
	                                     const std::vector<zone>* zones, const PT* keys, size_t n_keys) {
		const std::string who = "alp::gpu::column::sum_by_key_exact";
		if (!keys || n_keys == 0 || n_keys > ALPGPU_KEYED_MANY_KEYS_MAX) { throw std::runtime_error(who + ": 1 .. ALPGPU_KEYED_MANY_KEYS_MAX keys"); }
		uploaded_column val(blob_val, size_val, who.c_str()), key(blob_key, size_key, who.c_str());
		const uint64_t  nv = val.col.n_vectors;
		if (key.col.n_vectors != nv) { throw std::runtime_error(who + ": the columns differ in length"); }
		if (nv > ALPGPU_KEYED_EXACT_VECTORS_MAX) { throw std::runtime_error(who + ": at most ALPGPU_KEYED_EXACT_VECTORS_MAX vectors"); }
		if (mask && mask->size() != 16 * nv) { throw std::runtime_error(who + ": the mask must hold 16 words per vector"); }
		if (zones && zones->size() != nv) { throw std::runtime_error(who + ": one record per vector"); }
		keyed_result out;
		out.keys.assign(keys, keys + n_keys);
		std::sort(out.keys.begin(), out.keys.end(), [](PT a, PT b) { return b != b ? a == a : a < b; }); // ascending by <, NaNs last
		out.sums.assign(n_keys, 0.0);
		out.counts.assign(n_keys, 0);
		if (nv == 0) { return out; }
		const uint32_t nk       = static_cast<uint32_t>(n_keys);
		uint64_t*      d_mask   = mask ? static_cast<uint64_t*>(val.get(mask->size() * sizeof(uint64_t))) : nullptr;
		zone*          d_zones  = zones ? static_cast<zone*>(val.get(nv * sizeof(zone))) : nullptr;
		PT*            d_keys   = static_cast<PT*>(val.get(n_keys * sizeof(PT)));
		double*        d_sums   = static_cast<double*>(val.get(n_keys * sizeof(double)));
		uint64_t*      d_counts = static_cast<uint64_t*>(val.get((n_keys + 1) * sizeof(uint64_t)));
		void*          d_table  = val.get(alpgpu_keyed_exact_sum_table_bytes(nk));
		if (mask) { check(alpgpu_memcpy_h2d(context(), d_mask, mask->data(), mask->size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d"); }
		if (zones) { check(alpgpu_memcpy_h2d(context(), d_zones, zones->data(), nv * sizeof(zone)), "alpgpu_memcpy_h2d"); }
		check(alpgpu_memcpy_h2d(context(), d_keys, out.keys.data(), n_keys * sizeof(PT)), "alpgpu_memcpy_h2d");
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_decode_keyed_exact_sum_f64(context(), &val.col, &key.col, d_mask, d_zones, reinterpret_cast<const double*>(d_keys), nk, d_sums, d_counts, d_table, 0),
			      "alpgpu_decode_keyed_exact_sum_f64");
		} else {
			check(alpgpu_decode_keyed_exact_sum_f32(context(), &val.col, &key.col, d_mask, d_zones, reinterpret_cast<const float*>(d_keys), nk, d_sums, d_counts, d_table, 0),
			      "alpgpu_decode_keyed_exact_sum_f32");
		}
		std::vector<uint64_t> counts(n_keys + 1);
		check(alpgpu_memcpy_d2h(context(), out.sums.data(), d_sums, n_keys * sizeof(double)), "alpgpu_memcpy_d2h");
		check(alpgpu_memcpy_d2h(context(), counts.data(), d_counts, counts.size() * sizeof(uint64_t)), "alpgpu_memcpy_d2h");
		out.counts.assign(counts.begin(), counts.end() - 1);
		out.unmatched = counts.back();
		return out;
	}
	// Keyed MIN / MAX (include/alpgpu.h, "keyed MIN / MAX"): the record {min, max} and the COUNT of this column (blob val) per key, with sum_by_key's
	// arguments and key handling, for double and float columns (alpgpu_decode_keyed_minmax_*).  keys, records and counts come back in the order of
	// the sorted keys.  A record ignores NaN values (they are counted), orders -0.0 below +0.0 and is {+inf, -inf} for a key without a number and
	// for every later duplicate.  zones (optional): any records that contain the KEY vectors' intervals; they change no byte.
	struct keyed_minmax_result {
		std::vector<PT>       keys;
		std::vector<zone>     records;
		std::vector<uint64_t> counts;
		uint64_t              unmatched = 0;
	};
	static keyed_minmax_result minmax_by_key(const uint8_t* blob_val, size_t size_val, const uint8_t* blob_key, size_t size_key, const std::vector<uint64_t>* mask,
	                                         const std::vector<zone>* zones, const PT* keys, size_t n_keys) {
		return keyed_minmax_call(false, blob_val, size_val, blob_key, size_key, mask, zones, keys, n_keys);
	}
	// Keyed MIN / MAX for up to ALPGPU_KEYED_MANY_KEYS_MAX = 2^20 keys (include/alpgpu.h, "keyed MIN / MAX, many keys": alpgpu_decode_keyed_minmax_many_*):
	// minmax_by_key's arguments and result, the same bytes up to ALPGPU_KEYED_KEYS_MAX keys; the table sits in device memory, not in LDS.
	static keyed_minmax_result minmax_by_key_many(const uint8_t* blob_val, size_t size_val, const uint8_t* blob_key, size_t size_key, const std::vector<uint64_t>* mask,
	                                              const std::vector<zone>* zones, const PT* keys, size_t n_keys) {
		return keyed_minmax_call(true, blob_val, size_val, blob_key, size_key, mask, zones, keys, n_keys);
	}
	// what the two share: everything but the bound on n_keys and the entry point
	static keyed_minmax_result keyed_minmax_call(bool many, const uint8_t* blob_val, size_t size_val, const uint8_t* blob_key, size_t size_key, const std::vector<uint64_t>* mask,
	                                             const std::vector<zone>* zones, const PT* keys, size_t n_keys) {
		const std::string who = many ? "alp::gpu::column::minmax_by_key_many" : "alp::gpu::column::minmax_by_key";
		if (!keys || n_keys == 0 || n_keys > (many ? ALPGPU_KEYED_MANY_KEYS_MAX : ALPGPU_KEYED_KEYS_MAX)) {
			throw std::runtime_error(who + (many ? ": 1 .. ALPGPU_KEYED_MANY_KEYS_MAX keys" : ": 1 .. ALPGPU_KEYED_KEYS_MAX keys"));
		}
		uploaded_column val(blob_val, size_val, who.c_str()), key(blob_key, size_key, who.c_str());
		const uint64_t  nv = val.col.n_vectors;
		if (key.col.n_vectors != nv) { throw std::runtime_error(who + ": the columns differ in length"); }
		if (mask && mask->size() != 16 * nv) { throw std::runtime_error(who + ": the mask must hold 16 words per vector"); }
		if (zones && zones->size() != nv) { throw std::runtime_error(who + ": one record per vector"); }
		keyed_minmax_result out;
		out.keys.assign(keys, keys + n_keys);
		std::sort(out.keys.begin(), out.keys.end(), [](PT a, PT b) { return b != b ? a == a : a < b; }); // ascending by <, NaNs last
		zone none;
		none.min = std::numeric_limits<PT>::infinity();
		none.max = -std::numeric_limits<PT>::infinity();
		out.records.assign(n_keys, none);
		out.counts.assign(n_keys, 0);
		if (nv == 0) { return out; }
		uint64_t* d_mask   = mask ? static_cast<uint64_t*>(val.get(mask->size() * sizeof(uint64_t))) : nullptr;
		zone*     d_zones  = zones ? static_cast<zone*>(val.get(nv * sizeof(zone))) : nullptr;
		PT*       d_keys   = static_cast<PT*>(val.get(n_keys * sizeof(PT)));
		zone*     d_out    = static_cast<zone*>(val.get(n_keys * sizeof(zone)));
		uint64_t* d_counts = static_cast<uint64_t*>(val.get((n_keys + 1) * sizeof(uint64_t)));
		if (mask) { check(alpgpu_memcpy_h2d(context(), d_mask, mask->data(), mask->size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d"); }
		if (zones) { check(alpgpu_memcpy_h2d(context(), d_zones, zones->data(), nv * sizeof(zone)), "alpgpu_memcpy_h2d"); }
		check(alpgpu_memcpy_h2d(context(), d_keys, out.keys.data(), n_keys * sizeof(PT)), "alpgpu_memcpy_h2d");
		const uint32_t nk = static_cast<uint32_t>(n_keys);
		if constexpr (sizeof(PT) == 8) {
			const double* dk = reinterpret_cast<const double*>(d_keys);
			if (many) {
				check(alpgpu_decode_keyed_minmax_many_f64(context(), &val.col, &key.col, d_mask, d_zones, dk, nk, d_out, d_counts), "alpgpu_decode_keyed_minmax_many_f64");
			} else {
				check(alpgpu_decode_keyed_minmax_f64(context(), &val.col, &key.col, d_mask, d_zones, dk, nk, d_out, d_counts), "alpgpu_decode_keyed_minmax_f64");
			}
		} else {
			const float* dk = reinterpret_cast<const float*>(d_keys);
			if (many) {
				check(alpgpu_decode_keyed_minmax_many_f32(context(), &val.col, &key.col, d_mask, d_zones, dk, nk, d_out, d_counts), "alpgpu_decode_keyed_minmax_many_f32");
			} else {
				check(alpgpu_decode_keyed_minmax_f32(context(), &val.col, &key.col, d_mask, d_zones, dk, nk, d_out, d_counts), "alpgpu_decode_keyed_minmax_f32");
			}
		}
		std::vector<uint64_t> counts(n_keys + 1);
		check(alpgpu_memcpy_d2h(context(), out.records.data(), d_out, n_keys * sizeof(zone)), "alpgpu_memcpy_d2h");
		check(alpgpu_memcpy_d2h(context(), counts.data(), d_counts, counts.size() * sizeof(uint64_t)), "alpgpu_memcpy_d2h");
		out.counts.assign(counts.begin(), counts.end() - 1);
		out.unmatched = counts.back();
		return out;
	}
	// Bucketed aggregation (include/alpgpu.h, "bucketed aggregation"): SUM, or the record {min, max}, and the COUNT of this column (blob val) per bucket
	// of a key column of the same type and length (blob key; the same blob is allowed), over the rows whose bit is set in the mask (nullptr: all of
	// them), in one pass over the two columns (alpgpu_decode_bucket_sum_* / alpgpu_decode_bucket_minmax_*), for double and float columns.  edges:
	// 0 .. ALPGPU_BUCKET_EDGES_MAX edges, sorted here, on the host (NaNs last, where they are inert).  Bucket b holds the rows with b edges <= key
	// (right: < key): histogram's buckets.  sums / records: n_edges + 1; counts: the buckets' rows, as histogram(key) counts them; nan_keys: the
	// selected rows whose key is a NaN, which enter nothing else.  AVG is sums[b] / counts[b].  zones (optional): any records that contain the KEY
	// vectors' intervals; they change no byte.
	struct bucket_result {
		std::vector<PT>       edges;
		std::vector<double>   sums;    // sum_by_bucket
		std::vector<zone>     records; // minmax_by_bucket
		std::vector<uint64_t> counts;
		uint64_t              nan_keys = 0;
	};
	static bucket_result sum_by_bucket(const uint8_t* blob_val, size_t size_val, const uint8_t* blob_key, size_t size_key, const std::vector<uint64_t>* mask,
	                                   const std::vector<zone>* zones, const PT* edges, size_t n_edges, bool right = false) {
		return bucket_call(true, blob_val, size_val, blob_key, size_key, mask, zones, edges, n_edges, right);
	}
	static bucket_result minmax_by_bucket(const uint8_t* blob_val, size_t size_val, const uint8_t* blob_key, size_t size_key, const std::vector<uint64_t>* mask,
	                                      const std::vector<zone>* zones, const PT* edges, size_t n_edges, bool right = false) {
		return bucket_call(false, blob_val, size_val, blob_key, size_key, mask, zones, edges, n_edges, right);
	}
	// what the two share: everything but the result buffer and the entry point
	static bucket_result bucket_call(bool sum, const uint8_t* blob_val, size_t size_val, const uint8_t* blob_key, size_t size_key, const std::vector<uint64_t>* mask,
	                                 const std::vector<zone>* zones, const PT* edges, size_t n_edges, bool right) {
		const std::string who = sum ? "alp::gpu::column::sum_by_bucket" : "alp::gpu::column::minmax_by_bucket";
		if ((!edges && n_edges > 0) || n_edges > ALPGPU_BUCKET_EDGES_MAX) { throw std::runtime_error(who + ": 0 .. ALPGPU_BUCKET_EDGES_MAX edges"); }
		uploaded_column val(blob_val, size_val, who.c_str()), key(blob_key, size_key, who.c_str());
		const uint64_t  nv = val.col.n_vectors;
		if (key.col.n_vectors != nv) { throw std::runtime_error(who + ": the columns differ in length"); }
		if (mask && mask->size() != 16 * nv) { throw std::runtime_error(who + ": the mask must hold 16 words per vector"); }
		if (zones && zones->size() != nv) { throw std::runtime_error(who + ": one record per vector"); }
		const size_t  n_buckets = n_edges + 1;
		bucket_result out;
		if (n_edges > 0) { out.edges.assign(edges, edges + n_edges); }
		std::sort(out.edges.begin(), out.edges.end(), [](PT a, PT b) { return b != b ? a == a : a < b; }); // ascending by <, NaNs last
		zone none;
		none.min = std::numeric_limits<PT>::infinity();
		none.max = -std::numeric_limits<PT>::infinity();
		if (sum) { out.sums.assign(n_buckets, 0.0); } else { out.records.assign(n_buckets, none); }
		out.counts.assign(n_buckets, 0);
		if (nv == 0) { return out; }
		uint64_t* d_mask   = mask ? static_cast<uint64_t*>(val.get(mask->size() * sizeof(uint64_t))) : nullptr;
		zone*     d_zones  = zones ? static_cast<zone*>(val.get(nv * sizeof(zone))) : nullptr;
		PT*       d_edges  = n_edges > 0 ? static_cast<PT*>(val.get(n_edges * sizeof(PT))) : nullptr;
		void*     d_result = val.get(n_buckets * (sum ? sizeof(double) : sizeof(zone)));
		uint64_t* d_counts = static_cast<uint64_t*>(val.get((n_buckets + 1) * sizeof(uint64_t)));
		const uint32_t ne = static_cast<uint32_t>(n_edges);
		void*     d_scratch = sum ? val.get(alpgpu_bucket_sum_scratch_bytes(nv, ne)) : nullptr;
		if (mask) { check(alpgpu_memcpy_h2d(context(), d_mask, mask->data(), mask->size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d"); }
		if (zones) { check(alpgpu_memcpy_h2d(context(), d_zones, zones->data(), nv * sizeof(zone)), "alpgpu_memcpy_h2d"); }
		if (n_edges > 0) { check(alpgpu_memcpy_h2d(context(), d_edges, out.edges.data(), n_edges * sizeof(PT)), "alpgpu_memcpy_h2d"); }
		const int r = right ? 1 : 0;
		if constexpr (sizeof(PT) == 8) {
			const double* de = reinterpret_cast<const double*>(d_edges);
			if (sum) {
				check(alpgpu_decode_bucket_sum_f64(context(), &val.col, &key.col, d_mask, d_zones, de, ne, r, static_cast<double*>(d_result), d_counts, d_scratch), "alpgpu_decode_bucket_sum_f64");
			} else {
				check(alpgpu_decode_bucket_minmax_f64(context(), &val.col, &key.col, d_mask, d_zones, de, ne, r, static_cast<zone*>(d_result), d_counts), "alpgpu_decode_bucket_minmax_f64");
			}
		} else {
			const float* de = reinterpret_cast<const float*>(d_edges);
			if (sum) {
				check(alpgpu_decode_bucket_sum_f32(context(), &val.col, &key.col, d_mask, d_zones, de, ne, r, static_cast<double*>(d_result), d_counts, d_scratch), "alpgpu_decode_bucket_sum_f32");
			} else {
				check(alpgpu_decode_bucket_minmax_f32(context(), &val.col, &key.col, d_mask, d_zones, de, ne, r, static_cast<zone*>(d_result), d_counts), "alpgpu_decode_bucket_minmax_f32");
			}
		}
		std::vector<uint64_t> counts(n_buckets + 1);
		if (sum) {
			check(alpgpu_memcpy_d2h(context(), out.sums.data(), d_result, n_buckets * sizeof(double)), "alpgpu_memcpy_d2h");
		} else {
			check(alpgpu_memcpy_d2h(context(), out.records.data(), d_result, n_buckets * sizeof(zone)), "alpgpu_memcpy_d2h");
		}
		check(alpgpu_memcpy_d2h(context(), counts.data(), d_counts, counts.size() * sizeof(uint64_t)), "alpgpu_memcpy_d2h");
		out.counts.assign(counts.begin(), counts.end() - 1);
		out.nan_keys = counts.back();
		return out;
	}
	// Distinct values (include/alpgpu.h, "distinct values"): the distinct values, ascending, of the values [0, n_values) whose bit is set in the mask
	// (nullptr: all of them) and how often each occurs.  -0.0 == 0.0, one value, reported as +0.0; +-inf are ordinary; NaNs are no values and are only
	// counted (nans).  numbers = the selected values that are no NaNs: the sum of counts unless overflow.  overflow: there are more than `capacity`
	// (1 .. ALPGPU_DISTINCT_MAX) distinct values; values and counts are then empty: call again with a larger capacity.  The values are a valid sorted
	// list for select_in_mask, edge array for histogram and key array for join_probe.  zones (optional): any records that contain the vectors'
	// intervals; they change nothing.
	struct distinct_result {
		std::vector<PT>       values;
		std::vector<uint64_t> counts;
		uint64_t              nans = 0, numbers = 0;
		bool                  overflow = false;
	};
	static distinct_result distinct(const uint8_t* blob, size_t size, const std::vector<uint64_t>* mask = nullptr, const std::vector<zone>* zones = nullptr, uint64_t capacity = 65536) {
		if (capacity == 0 || capacity > ALPGPU_DISTINCT_MAX) { throw std::runtime_error("alp::gpu::column::distinct: the capacity must be in 1 .. ALPGPU_DISTINCT_MAX"); }
		uploaded_column up(blob, size, "alp::gpu::column::distinct");
		const uint64_t  nv = up.col.n_vectors;
		if (mask && mask->size() != 16 * nv) { throw std::runtime_error("alp::gpu::column::distinct: the mask must hold 16 words per vector"); }
		if (zones && zones->size() != nv) { throw std::runtime_error("alp::gpu::column::distinct: one record per vector"); }
		distinct_result out;
		if (nv == 0) { return out; }
		uint64_t* d_mask    = mask ? static_cast<uint64_t*>(up.get(mask->size() * sizeof(uint64_t))) : nullptr;
		zone*     d_zones   = zones ? static_cast<zone*>(up.get(nv * sizeof(zone))) : nullptr;
		PT*       d_vals    = static_cast<PT*>(up.get(capacity * sizeof(PT)));
		uint64_t* d_counts  = static_cast<uint64_t*>(up.get(capacity * sizeof(uint64_t)));
		uint64_t* d_state   = static_cast<uint64_t*>(up.get(4 * sizeof(uint64_t)));
		void*     d_scratch = up.get(alpgpu_distinct_scratch_bytes(capacity));
		if (mask) { check(alpgpu_memcpy_h2d(context(), d_mask, mask->data(), mask->size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d"); }
		if (zones) { check(alpgpu_memcpy_h2d(context(), d_zones, zones->data(), nv * sizeof(zone)), "alpgpu_memcpy_h2d"); }
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_distinct_f64(context(), &up.col, 0, up.n_values, d_mask, d_zones, capacity, reinterpret_cast<double*>(d_vals), d_counts, d_state, d_scratch), "alpgpu_distinct_f64");
		} else {
			check(alpgpu_distinct_f32(context(), &up.col, 0, up.n_values, d_mask, d_zones, capacity, reinterpret_cast<float*>(d_vals), d_counts, d_state, d_scratch), "alpgpu_distinct_f32");
		}
		uint64_t state[4] = {0, 0, 0, 0};
		check(alpgpu_memcpy_d2h(context(), state, d_state, sizeof(state)), "alpgpu_memcpy_d2h");
		out.nans     = state[1];
		out.numbers  = state[2];
		out.overflow = state[3] != 0;
		if (out.overflow || state[0] == 0) { return out; }
		out.values.resize(state[0]);
		out.counts.resize(state[0]);
		check(alpgpu_memcpy_d2h(context(), out.values.data(), d_vals, state[0] * sizeof(PT)), "alpgpu_memcpy_d2h");
		check(alpgpu_memcpy_d2h(context(), out.counts.data(), d_counts, state[0] * sizeof(uint64_t)), "alpgpu_memcpy_d2h");
		return out;
	}
	// Join probe (include/alpgpu.h, "join probe"): one row per set bit of the mask (nullptr: every value of [0, n_vectors * 1024)), ascending by index.
	// pos[j] = the position IN `keys` AS PASSED of a key == the row's value (-0.0 == 0.0, a NaN never matches), ALPGPU_JOIN_NO_MATCH where there is
	// none; span[j] = the number of keys == it; indices[j] = the row's value index.  The keys are sorted here, on the host (stably, NaNs last), and the
	// sort's permutation goes along as the call's d_rows: among equal keys pos is the first of them in `keys`.  zones (optional): any records that
	// contain the vectors' intervals; they change no row.
	struct join_result {
		std::vector<int64_t>  pos, indices;
		std::vector<uint32_t> span;
	};
	static join_result join_probe(const uint8_t* blob, size_t size, const std::vector<PT>& keys, const std::vector<uint64_t>* mask = nullptr, const std::vector<zone>* zones = nullptr) {
		if (keys.size() > 0x7FFFFFFFull) { throw std::runtime_error("alp::gpu::column::join_probe: at most 2^31 - 1 keys"); }
		uploaded_column up(blob, size, "alp::gpu::column::join_probe");
		const uint64_t  nv = up.col.n_vectors;
		if (mask && mask->size() != 16 * nv) { throw std::runtime_error("alp::gpu::column::join_probe: the mask must hold 16 words per vector"); }
		if (zones && zones->size() != nv) { throw std::runtime_error("alp::gpu::column::join_probe: one record per vector"); }
		join_result out;
		if (nv == 0) { return out; }
		std::vector<int64_t> rows(keys.size());
		for (size_t i = 0; i < rows.size(); ++i) { rows[i] = static_cast<int64_t>(i); }
		std::stable_sort(rows.begin(), rows.end(), [&](int64_t a, int64_t b) { return keys[b] != keys[b] ? keys[a] == keys[a] : keys[a] < keys[b]; }); // ascending by <, NaNs last
		std::vector<PT> list(keys.size());
		for (size_t i = 0; i < rows.size(); ++i) { list[i] = keys[static_cast<size_t>(rows[i])]; }
		uint64_t* d_mask    = mask ? static_cast<uint64_t*>(up.get(mask->size() * sizeof(uint64_t))) : nullptr;
		zone*     d_zones   = zones ? static_cast<zone*>(up.get(nv * sizeof(zone))) : nullptr;
		PT*       d_keys    = list.empty() ? nullptr : static_cast<PT*>(up.get(list.size() * sizeof(PT)));
		int64_t*  d_rows    = list.empty() ? nullptr : static_cast<int64_t*>(up.get(rows.size() * sizeof(int64_t)));
		uint64_t* d_count   = static_cast<uint64_t*>(up.get(sizeof(uint64_t)));
		void*     d_scratch = mask ? up.get(alpgpu_select_scratch_bytes(nv)) : nullptr;
		if (mask) { check(alpgpu_memcpy_h2d(context(), d_mask, mask->data(), mask->size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d"); }
		if (zones) { check(alpgpu_memcpy_h2d(context(), d_zones, zones->data(), nv * sizeof(zone)), "alpgpu_memcpy_h2d"); }
		if (d_keys) {
			check(alpgpu_memcpy_h2d(context(), d_keys, list.data(), list.size() * sizeof(PT)), "alpgpu_memcpy_h2d");
			check(alpgpu_memcpy_h2d(context(), d_rows, rows.data(), rows.size() * sizeof(int64_t)), "alpgpu_memcpy_h2d");
		}
		const auto probe = [&](int64_t* d_pos, uint32_t* d_span, int64_t* d_idx, uint64_t capacity) {
			if constexpr (sizeof(PT) == 8) {
				return alpgpu_join_probe_f64(context(), &up.col, d_mask, d_zones, reinterpret_cast<const double*>(d_keys), list.size(), d_rows, d_pos, d_span, d_idx, capacity, d_count, d_scratch);
			} else {
				return alpgpu_join_probe_f32(context(), &up.col, d_mask, d_zones, reinterpret_cast<const float*>(d_keys), list.size(), d_rows, d_pos, d_span, d_idx, capacity, d_count, d_scratch);
			}
		};
		uint64_t count = 0;
		check(probe(nullptr, nullptr, nullptr, 0), "alpgpu_join_probe"); // count first, then allocate exactly
		check(alpgpu_memcpy_d2h(context(), &count, d_count, sizeof(count)), "alpgpu_memcpy_d2h");
		if (count == 0) { return out; }
		int64_t*  d_pos  = static_cast<int64_t*>(up.get(count * sizeof(int64_t)));
		int64_t*  d_idx  = static_cast<int64_t*>(up.get(count * sizeof(int64_t)));
		uint32_t* d_span = static_cast<uint32_t*>(up.get(count * sizeof(uint32_t)));
		check(probe(d_pos, d_span, d_idx, count), "alpgpu_join_probe");
		out.pos.resize(count);
		out.indices.resize(count);
		out.span.resize(count);
		check(alpgpu_memcpy_d2h(context(), out.pos.data(), d_pos, count * sizeof(int64_t)), "alpgpu_memcpy_d2h");
		check(alpgpu_memcpy_d2h(context(), out.indices.data(), d_idx, count * sizeof(int64_t)), "alpgpu_memcpy_d2h");
		check(alpgpu_memcpy_d2h(context(), out.span.data(), d_span, count * sizeof(uint32_t)), "alpgpu_memcpy_d2h");
		return out;
	}
	// The column's values at the set bits of the mask, ascending by index (alpgpu_decode_masked_*): each with the bits decompress gives it.  The
	// second form also fills `indices` with their value indices (what mask_indices returns).
	static std::vector<PT> take_masked(const uint8_t* blob, size_t size, const std::vector<uint64_t>& mask) { return take_masked_with(blob, size, mask, nullptr); }
	static std::vector<PT> take_masked(const uint8_t* blob, size_t size, const std::vector<uint64_t>& mask, std::vector<int64_t>& indices) {
		return take_masked_with(blob, size, mask, &indices);
	}

private:
	static std::vector<PT> take_masked_with(const uint8_t* blob, size_t size, const std::vector<uint64_t>& mask, std::vector<int64_t>* indices) {
		uploaded_column up(blob, size, "alp::gpu::column::take_masked");
		const uint64_t  nv = up.col.n_vectors;
		if (mask.size() != 16 * nv) { throw std::runtime_error("alp::gpu::column::take_masked: the mask must hold 16 words per vector"); }
		std::vector<PT> out;
		if (indices) { indices->clear(); }
		if (nv == 0) { return out; }
		uint64_t* d_mask    = static_cast<uint64_t*>(up.get(mask.size() * sizeof(uint64_t)));
		uint64_t* d_count   = static_cast<uint64_t*>(up.get(sizeof(uint64_t)));
		void*     d_scratch = up.get(alpgpu_select_scratch_bytes(nv));
		check(alpgpu_memcpy_h2d(context(), d_mask, mask.data(), mask.size() * sizeof(uint64_t)), "alpgpu_memcpy_h2d");
		uint64_t count = 0;
		check(decode_masked(&up.col, d_mask, nullptr, nullptr, 0, d_count, d_scratch), "alpgpu_decode_masked"); // count first, then allocate exactly
		check(alpgpu_memcpy_d2h(context(), &count, d_count, sizeof(count)), "alpgpu_memcpy_d2h");
		if (count == 0) { return out; }
		PT*      d_vals = static_cast<PT*>(up.get(count * sizeof(PT)));
		int64_t* d_idx  = indices ? static_cast<int64_t*>(up.get(count * sizeof(int64_t))) : nullptr;
		check(decode_masked(&up.col, d_mask, d_vals, d_idx, count, d_count, d_scratch), "alpgpu_decode_masked");
		out.resize(count);
		check(alpgpu_memcpy_d2h(context(), out.data(), d_vals, count * sizeof(PT)), "alpgpu_memcpy_d2h");
		if (indices) {
			indices->resize(count);
			check(alpgpu_memcpy_d2h(context(), indices->data(), d_idx, count * sizeof(int64_t)), "alpgpu_memcpy_d2h");
		}
		return out;
	}
	static int decode_masked(const alpgpu_column* col, const uint64_t* d_mask, PT* d_vals, int64_t* d_idx, uint64_t capacity, uint64_t* d_count, void* d_scratch) {
		if constexpr (sizeof(PT) == 8) {
			return alpgpu_decode_masked_f64(context(), col, d_mask, reinterpret_cast<double*>(d_vals), d_idx, capacity, d_count, d_scratch);
		} else {
			return alpgpu_decode_masked_f32(context(), col, d_mask, reinterpret_cast<float*>(d_vals), d_idx, capacity, d_count, d_scratch);
		}
	}
	static void select_mask_with(const uint8_t* blob, size_t size, PT lo, PT hi, mask_op op, std::vector<uint64_t>& mask, bool fresh) {
		uploaded_column up(blob, size, "alp::gpu::column::select_mask");
		const uint64_t  words = 16 * up.col.n_vectors;
		if (fresh) {
			mask.assign(words, 0);
		} else if (mask.size() != words) {
			throw std::runtime_error("alp::gpu::column::select_mask: the mask must hold 16 words per vector");
		}
		if (words == 0) { return; }
		uint64_t* d_mask = static_cast<uint64_t*>(up.get(words * sizeof(uint64_t)));
		if (op != mask_set) { check(alpgpu_memcpy_h2d(context(), d_mask, mask.data(), words * sizeof(uint64_t)), "alpgpu_memcpy_h2d"); }
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_select_mask_f64(context(), &up.col, 0, up.n_values, lo, hi, op, d_mask), "alpgpu_select_mask_f64");
		} else {
			check(alpgpu_select_mask_f32(context(), &up.col, 0, up.n_values, lo, hi, op, d_mask), "alpgpu_select_mask_f32");
		}
		check(alpgpu_memcpy_d2h(context(), mask.data(), d_mask, words * sizeof(uint64_t)), "alpgpu_memcpy_d2h");
	}
	static void select_in_mask_with(const uint8_t* blob, size_t size, const std::vector<PT>& values, bool negate, mask_op op, std::vector<uint64_t>& mask, bool fresh) {
		uploaded_column up(blob, size, "alp::gpu::column::select_in_mask");
		const uint64_t  words = 16 * up.col.n_vectors;
		if (fresh) {
			mask.assign(words, 0);
		} else if (mask.size() != words) {
			throw std::runtime_error("alp::gpu::column::select_in_mask: the mask must hold 16 words per vector");
		}
		if (words == 0) { return; }
		std::vector<PT> list(values);
		std::sort(list.begin(), list.end(), [](PT a, PT b) { return b != b ? a == a : a < b; }); // ascending by <, NaNs last
		uint64_t* d_mask = static_cast<uint64_t*>(up.get(words * sizeof(uint64_t)));
		PT*       d_list = list.empty() ? nullptr : static_cast<PT*>(up.get(list.size() * sizeof(PT)));
		if (op != mask_set) { check(alpgpu_memcpy_h2d(context(), d_mask, mask.data(), words * sizeof(uint64_t)), "alpgpu_memcpy_h2d"); }
		if (d_list) { check(alpgpu_memcpy_h2d(context(), d_list, list.data(), list.size() * sizeof(PT)), "alpgpu_memcpy_h2d"); }
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_select_in_mask_f64(context(), &up.col, 0, up.n_values, reinterpret_cast<const double*>(d_list), list.size(), negate ? 1 : 0, nullptr, op, d_mask), "alpgpu_select_in_mask_f64");
		} else {
			check(alpgpu_select_in_mask_f32(context(), &up.col, 0, up.n_values, reinterpret_cast<const float*>(d_list), list.size(), negate ? 1 : 0, nullptr, op, d_mask), "alpgpu_select_in_mask_f32");
		}
		check(alpgpu_memcpy_d2h(context(), mask.data(), d_mask, words * sizeof(uint64_t)), "alpgpu_memcpy_d2h");
	}
	static void compare_mask_with(const uint8_t* blob_a, size_t size_a, const uint8_t* blob_b, size_t size_b, compare_op cmp, mask_op op, std::vector<uint64_t>& mask, bool fresh) {
		uploaded_column a(blob_a, size_a, "alp::gpu::column::compare_mask"), b(blob_b, size_b, "alp::gpu::column::compare_mask");
		if (b.col.n_vectors != a.col.n_vectors || b.n_values != a.n_values) { throw std::runtime_error("alp::gpu::column::compare_mask: the columns differ in length"); }
		const uint64_t words = 16 * a.col.n_vectors;
		if (fresh) {
			mask.assign(words, 0);
		} else if (mask.size() != words) {
			throw std::runtime_error("alp::gpu::column::compare_mask: the mask must hold 16 words per vector");
		}
		if (words == 0) { return; }
		uint64_t* d_mask = static_cast<uint64_t*>(a.get(words * sizeof(uint64_t)));
		if (op != mask_set) { check(alpgpu_memcpy_h2d(context(), d_mask, mask.data(), words * sizeof(uint64_t)), "alpgpu_memcpy_h2d"); }
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_compare_mask_f64(context(), &a.col, &b.col, 0, a.n_values, cmp, op, d_mask), "alpgpu_compare_mask_f64");
		} else {
			check(alpgpu_compare_mask_f32(context(), &a.col, &b.col, 0, a.n_values, cmp, op, d_mask), "alpgpu_compare_mask_f32");
		}
		check(alpgpu_memcpy_d2h(context(), mask.data(), d_mask, words * sizeof(uint64_t)), "alpgpu_memcpy_d2h");
	}
	static void make_zone_map(uploaded_column& up, zone* d_zones) {
		if constexpr (sizeof(PT) == 8) {
			check(alpgpu_zone_map_f64(context(), &up.col, d_zones), "alpgpu_zone_map_f64");
		} else {
			check(alpgpu_zone_map_f32(context(), &up.col, d_zones), "alpgpu_zone_map_f32");
		}
	}
	static selection select_range_with(const uint8_t* blob, size_t size, PT lo, PT hi, const std::vector<zone>* zones) {
		uploaded_column up(blob, size, "alp::gpu::column::select_range");
		selection       out;
		if (up.n_values == 0) { return out; }
		uint64_t* d_count   = static_cast<uint64_t*>(up.get(sizeof(uint64_t)));
		void*     d_scratch = up.get(alpgpu_select_scratch_bytes(up.col.n_vectors));
		zone*     d_zones   = nullptr;
		if (zones != nullptr) {
			d_zones = static_cast<zone*>(up.get(zones->size() * sizeof(zone)));
			check(alpgpu_memcpy_h2d(context(), d_zones, zones->data(), zones->size() * sizeof(zone)), "alpgpu_memcpy_h2d");
		}
		auto      call      = [&](int64_t* d_idx, PT* d_vals, uint64_t capacity) {
			if (d_zones != nullptr) {
				if constexpr (sizeof(PT) == 8) {
					check(alpgpu_select_range_zoned_f64(context(), &up.col, d_zones, 0, up.n_values, lo, hi, d_idx, reinterpret_cast<double*>(d_vals), capacity, d_count, d_scratch),
					      "alpgpu_select_range_zoned_f64");
				} else {
					check(alpgpu_select_range_zoned_f32(context(), &up.col, d_zones, 0, up.n_values, lo, hi, d_idx, reinterpret_cast<float*>(d_vals), capacity, d_count, d_scratch),
					      "alpgpu_select_range_zoned_f32");
				}
				return;
			}
			if constexpr (sizeof(PT) == 8) {
				check(alpgpu_select_range_f64(context(), &up.col, 0, up.n_values, lo, hi, d_idx, reinterpret_cast<double*>(d_vals), capacity, d_count, d_scratch),
				      "alpgpu_select_range_f64");
			} else {
				check(alpgpu_select_range_f32(context(), &up.col, 0, up.n_values, lo, hi, d_idx, reinterpret_cast<float*>(d_vals), capacity, d_count, d_scratch),
				      "alpgpu_select_range_f32");
			}
		};
		uint64_t count = 0;
		call(nullptr, nullptr, 0); // count first, then allocate exactly
		check(alpgpu_memcpy_d2h(context(), &count, d_count, sizeof(count)), "alpgpu_memcpy_d2h");
		if (count == 0) { return out; }
		int64_t* d_idx  = static_cast<int64_t*>(up.get(count * sizeof(int64_t)));
		PT*      d_vals = static_cast<PT*>(up.get(count * sizeof(PT)));
		call(d_idx, d_vals, count);
		out.indices.resize(count);
		out.values.resize(count);
		check(alpgpu_memcpy_d2h(context(), out.indices.data(), d_idx, count * sizeof(int64_t)), "alpgpu_memcpy_d2h");
		check(alpgpu_memcpy_d2h(context(), out.values.data(), d_vals, count * sizeof(PT)), "alpgpu_memcpy_d2h");
		return out;
	}
};

}} // namespace alp::gpu
#endif
