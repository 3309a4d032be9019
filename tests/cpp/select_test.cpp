// select_test.cpp — alp::gpu::column<PT>::select_range (include/alp/batch.hpp): the values of a serialized column inside [lo, hi] and their value
// indices, selected on the GPU from the compressed column (include/alpgpu.h: alpgpu_select_range_*), against a scan of
// alp::gpu::column<PT>::decompress of the same blob on the host, bit for bit.  Double and float columns with ALP and ALP_RD rowgroups, exceptions
// and specials and an incomplete last vector (whose padding must never qualify); a band, a point, everything, nothing, a NaN bound; a blob too
// short for its header throws; a blob whose descriptors alpgpu_column_from_blob* refuses throws from select_range and from take, and every device
// buffer allocated for it by then is freed again (this program's own alpgpu_malloc / alpgpu_free stand in front of the library's and count).
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/select_test.cpp -Lalp_amd -lalpgpu -ldl && ./a.out
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <stdexcept>
#include <vector>

#include "alp.hpp"
#include "alp/batch.hpp"

// The header allocates through alpgpu_malloc / alpgpu_free.  Defined here, they are the ones every caller in the process binds to; they count the
// buffers alive and pass the call on to the library's own.
static long live_buffers = 0;
extern "C" int alpgpu_malloc(alpgpu_ctx* ctx, void** d_ptr, size_t bytes) {
	static const auto real = reinterpret_cast<int (*)(alpgpu_ctx*, void**, size_t)>(dlsym(RTLD_NEXT, "alpgpu_malloc"));
	const int         rc   = real(ctx, d_ptr, bytes);
	live_buffers += rc == 0;
	return rc;
}
extern "C" int alpgpu_free(alpgpu_ctx* ctx, void* d_ptr) {
	static const auto real = reinterpret_cast<int (*)(alpgpu_ctx*, void*)>(dlsym(RTLD_NEXT, "alpgpu_free"));
	live_buffers -= d_ptr != nullptr;
	return real(ctx, d_ptr);
}

static int failures = 0;
#define EXPECT(cond, ...)                                                                                              \
	do {                                                                                                               \
		if (!(cond)) {                                                                                                 \
			++failures;                                                                                                \
			std::printf("FAIL %s:%d: ", __FILE__, __LINE__);                                                           \
			std::printf(__VA_ARGS__);                                                                                  \
			std::printf("\n");                                                                                         \
		}                                                                                                              \
	} while (0)

template <class PT>
std::vector<PT> make_column(size_t n_values, unsigned seed) {
	std::mt19937_64                        rng(seed);
	std::uniform_real_distribution<double> uni(-1e4, 1e4), unit(0.0, 1.0);
	std::vector<PT>                        v(n_values);
	for (size_t i = 0; i < n_values; ++i) {
		const size_t rg = i / (100 * 1024);
		if (rg % 2 == 1) {
			v[i] = static_cast<PT>(unit(rng)); // full precision: ALP_RD rowgroups
		} else {
			v[i] = static_cast<PT>(std::round(uni(rng) * 100.0) / 100.0);
			if ((rng() & 127) == 0) { v[i] = static_cast<PT>(uni(rng) * 3.14159265358979); }
			if ((rng() & 1023) == 0) { v[i] = (rng() & 1) ? -0.0 : std::numeric_limits<PT>::quiet_NaN(); }
		}
	}
	return v;
}

template <class PT, class U>
void check_range(const char* name, const std::vector<uint8_t>& blob, const std::vector<PT>& all, size_t n_values, PT lo, PT hi, bool want_some) {
	const auto            got = alp::gpu::column<PT>::select_range(blob.data(), blob.size(), lo, hi);
	std::vector<uint64_t> idx;
	for (size_t i = 0; i < n_values; ++i) {
		if (all[i] >= lo && all[i] <= hi) { idx.push_back(i); }
	}
	EXPECT(got.indices.size() == idx.size() && got.values.size() == idx.size(), "%s [%g, %g]: %zu indices, %zu values, expected %zu", name, double(lo), double(hi),
	       got.indices.size(), got.values.size(), idx.size());
	EXPECT(!want_some || (!idx.empty() && idx.size() < n_values), "%s [%g, %g]: the case selects %zu of %zu values", name, double(lo), double(hi), idx.size(), n_values);
	size_t bad = 0;
	for (size_t k = 0; k < idx.size() && k < got.indices.size() && k < got.values.size(); ++k) {
		U a, b;
		std::memcpy(&a, &got.values[k], sizeof(U));
		std::memcpy(&b, &all[idx[k]], sizeof(U));
		bad += got.indices[k] != idx[k] || a != b;
	}
	EXPECT(bad == 0, "%s [%g, %g]: %zu selected entries differ from a scan of decompress", name, double(lo), double(hi), bad);
}

template <class PT, class U>
void run(const char* name, size_t n_values, unsigned seed) {
	const std::vector<PT>      col  = make_column<PT>(n_values, seed);
	const std::vector<uint8_t> blob = alp::gpu::column<PT>::compress(col.data(), col.size());
	const std::vector<PT>      all  = alp::gpu::column<PT>::decompress(blob.data(), blob.size());
	const PT                   inf  = std::numeric_limits<PT>::infinity();
	check_range<PT, U>(name, blob, all, n_values, PT(-250.5), PT(1234.25), true); // a band across the ALP rowgroups and all of the ALP_RD ones
	check_range<PT, U>(name, blob, all, n_values, PT(0.25), PT(0.26), true);      // a narrow band inside the ALP_RD values
	check_range<PT, U>(name, blob, all, n_values, PT(0), PT(0), false);           // -0.0 and +0.0
	check_range<PT, U>(name, blob, all, n_values, col[n_values / 1024 * 1024], col[n_values / 1024 * 1024], true); // the padding's value: the padding itself must stay out
	check_range<PT, U>(name, blob, all, n_values, -inf, inf, true);               // everything but the NaNs
	check_range<PT, U>(name, blob, all, n_values, PT(5), PT(-5), false);
	check_range<PT, U>(name, blob, all, n_values, std::numeric_limits<PT>::quiet_NaN(), inf, false);
	bool threw = false;
	try {
		alp::gpu::column<PT>::select_range(blob.data(), 40, PT(0), PT(1));
	} catch (const std::exception&) { threw = true; }
	EXPECT(threw, "%s: a blob shorter than its header did not throw", name);
	// A blob that is refused AFTER the device buffers for it were allocated: the last vector's bit width (byte 24 of its 32-byte descriptor) made
	// impossible.  Every refused call would otherwise leave about a blob's worth of device memory behind.
	alpgpu_blob_header h;
	std::memcpy(&h, blob.data(), sizeof(h));
	std::vector<uint8_t> bad = blob;
	bad[sizeof(h) + 32 * h.n_rowgroups + 32 * (h.n_vectors - 1) + 24] = 200;
	const uint64_t idx[2] = {0, 5};
	alp::gpu::column<PT>::take(blob.data(), blob.size(), idx, 2); // (whatever the process allocates once and keeps is there by now)
	const long live0  = live_buffers;
	int        thrown = 0;
	for (int i = 0; i < 3; ++i) {
		try {
			alp::gpu::column<PT>::select_range(bad.data(), bad.size(), PT(0), PT(1));
		} catch (const std::exception&) { ++thrown; }
		try {
			alp::gpu::column<PT>::take(bad.data(), bad.size(), idx, 2);
		} catch (const std::exception&) { ++thrown; }
	}
	EXPECT(thrown == 6, "%s: a blob with an impossible descriptor threw %d times out of 6", name, thrown);
	EXPECT(live_buffers == live0, "%s: %ld device buffers left allocated by 6 refused blobs", name, live_buffers - live0);
	alp::gpu::column<PT>::select_range(blob.data(), blob.size(), PT(0), PT(1));
	EXPECT(live_buffers == live0, "%s: %ld device buffers left allocated by a select_range", name, live_buffers - live0);
	std::printf("%s: %zu values\n", name, n_values);
}

int main() {
	run<double, uint64_t>("double", 250 * 1024 + 333, 5);
	run<float, uint32_t>("float", 230 * 1024 + 77, 6);
	std::printf("select_test: %d failures\n", failures);
	return failures ? 1 : 0;
}
