// zone_test.cpp — alp::gpu::column<PT>::zone_map, min_max and select_range with a zone map (include/alp/batch.hpp; include/alpgpu.h, "zone
// maps"), against alp::gpu::column<PT>::decompress of the same blob scanned on the host.  Expected record of a vector: minimum and maximum of the
// order-preserving integer key of its values that are not NaN (-0.0 below +0.0), {+inf, -inf} when there is none; compared bit for bit.  The
// zoned selection must equal the plain one for exact records, widened records and {-inf, +inf} everywhere.  A random column (ALP and ALP_RD
// rowgroups, exceptions, NaNs, zeros of both signs, a vector of NaNs only, an incomplete last vector) and a sorted one, double and float; a
// zone map of the wrong length throws; no device buffer is left behind.
//   g++ -std=c++17 -O1 -Iinclude tests/cpp/zone_test.cpp -Lalp_amd -lalpgpu -ldl && ./a.out
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <stdexcept>
#include <type_traits>
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
using bits_t = typename std::conditional<sizeof(PT) == 8, int64_t, int32_t>::type;

template <class PT>
bits_t<PT> bits_of(PT x) {
	bits_t<PT> b;
	std::memcpy(&b, &x, sizeof(b));
	return b;
}
template <class PT>
bits_t<PT> key_of(PT x) {
	const bits_t<PT> b = bits_of(x);
	return b >= 0 ? b : b ^ std::numeric_limits<bits_t<PT>>::max();
}

template <class PT>
std::vector<PT> random_column(size_t n_values, unsigned seed) {
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
		}
		if ((rng() & 1023) == 0) { v[i] = (rng() & 1) ? PT(-0.0) : std::numeric_limits<PT>::quiet_NaN(); }
	}
	for (size_t i = 5 * 1024; i < 6 * 1024 && i < n_values; ++i) { v[i] = std::numeric_limits<PT>::quiet_NaN(); } // a vector of NaNs only
	for (size_t i = 7 * 1024; i < 8 * 1024 && i < n_values; ++i) { v[i] = (i & 1) ? PT(0.0) : PT(-0.0); }       // a vector of zeros of both signs
	return v;
}

template <class PT>
std::vector<PT> sorted_column(size_t n_values, unsigned seed) {
	std::mt19937_64                        rng(seed);
	std::uniform_real_distribution<double> uni(-1e4, 1e4);
	std::vector<PT>                        v(n_values);
	for (auto& x : v) { x = static_cast<PT>(std::round(uni(rng) * 10.0) / 10.0); }
	std::sort(v.begin(), v.end());
	return v;
}

template <class PT>
bool same_selection(const typename alp::gpu::column<PT>::selection& a, const typename alp::gpu::column<PT>::selection& b) {
	return a.indices == b.indices && a.values.size() == b.values.size() && (a.values.empty() || std::memcmp(a.values.data(), b.values.data(), a.values.size() * sizeof(PT)) == 0);
}

template <class PT>
void run(const char* name, const std::vector<PT>& col, size_t min_excluded) {
	using column = alp::gpu::column<PT>;
	using zone   = typename column::zone;
	static_assert(sizeof(zone) == 2 * sizeof(PT), "a record is {min, max}");
	const size_t               n_values = col.size();
	const std::vector<uint8_t> blob     = column::compress(col.data(), col.size());
	const std::vector<PT>      all      = column::decompress(blob.data(), blob.size());
	const PT                   inf      = std::numeric_limits<PT>::infinity();
	const long                 live0    = (column::zone_map(blob.data(), blob.size()), live_buffers); // (whatever the process allocates once and keeps is there by now)
	const std::vector<zone>    zones    = column::zone_map(blob.data(), blob.size());
	const size_t               n_vec    = (n_values + 1023) / 1024;
	EXPECT(zones.size() == n_vec, "%s: %zu records for %zu vectors", name, zones.size(), n_vec);
	// every record against a host scan of the decompressed values; the padding repeats a value of its vector, so the scan stops at n_values
	size_t bad = 0;
	PT     cmin = inf, cmax = -inf;
	bool   seen = false;
	for (size_t v = 0; v < n_vec && v < zones.size(); ++v) {
		PT   mn = inf, mx = -inf;
		bool any = false;
		for (size_t i = v * 1024; i < std::min(n_values, (v + 1) * 1024); ++i) {
			if (all[i] != all[i]) { continue; }
			if (!any || key_of(all[i]) < key_of(mn)) { mn = all[i]; }
			if (!any || key_of(all[i]) > key_of(mx)) { mx = all[i]; }
			any = true;
		}
		bad += bits_of(zones[v].min) != bits_of(mn) || bits_of(zones[v].max) != bits_of(mx);
		if (any) {
			if (!seen || key_of(mn) < key_of(cmin)) { cmin = mn; }
			if (!seen || key_of(mx) > key_of(cmax)) { cmax = mx; }
			seen = true;
		}
	}
	EXPECT(bad == 0, "%s: %zu records differ from a scan of decompress", name, bad);
	const zone mm = column::min_max(blob.data(), blob.size());
	EXPECT(bits_of(mm.min) == bits_of(cmin) && bits_of(mm.max) == bits_of(cmax), "%s: min_max {%g, %g}, expected {%g, %g}", name, double(mm.min), double(mm.max), double(cmin),
	       double(cmax));
	// the zoned selection equals the plain one: exact records, widened ones, {-inf, +inf} everywhere
	std::vector<zone> wide = zones, open = zones;
	std::mt19937_64   rng(11);
	for (auto& z : wide) {
		if (z.min <= z.max) {
			z.min = std::nextafter(z.min - PT(rng() % 7), -inf);
			z.max = std::nextafter(z.max + PT(rng() % 7), inf);
		}
	}
	for (auto& z : open) { z.min = -inf, z.max = inf; }
	PT q0 = all[n_values / 2 - 700], q1 = all[n_values / 2]; // a band about 700 values wide in a sorted column
	if (q0 != q0) { q0 = PT(0); }
	if (q1 != q1) { q1 = PT(0); }
	const PT preds[][2] = {{PT(-250.5), PT(1234.25)}, {PT(0.25), PT(0.26)}, {PT(0), PT(0)}, {std::min(q0, q1), std::max(q0, q1)}, {-inf, inf}, {PT(5), PT(-5)},
	                       {std::numeric_limits<PT>::quiet_NaN(), inf}, {col[n_values / 1024 * 1024], col[n_values / 1024 * 1024]}};
	size_t some = 0;
	for (const auto& p : preds) {
		const auto plain = column::select_range(blob.data(), blob.size(), p[0], p[1]);
		size_t     expect = 0;
		for (size_t i = 0; i < n_values; ++i) { expect += all[i] >= p[0] && all[i] <= p[1]; }
		EXPECT(plain.indices.size() == expect, "%s [%g, %g]: plain select %zu, scan %zu", name, double(p[0]), double(p[1]), plain.indices.size(), expect);
		some += expect > 0 && expect < n_values;
		for (const std::vector<zone>* z : {&zones, static_cast<const std::vector<zone>*>(&wide), static_cast<const std::vector<zone>*>(&open)}) {
			const auto got = column::select_range(blob.data(), blob.size(), p[0], p[1], *z);
			EXPECT(same_selection<PT>(got, plain), "%s [%g, %g]: zoned select (%zu) differs from the plain one (%zu)", name, double(p[0]), double(p[1]), got.indices.size(),
			       plain.indices.size());
		}
	}
	EXPECT(some >= 3, "%s: only %zu predicates select some but not all values", name, some);
	size_t excluded = 0;
	const PT lo = std::min(q0, q1), hi = std::max(q0, q1);
	for (const auto& z : zones) { excluded += !(z.max >= lo && z.min <= hi); }
	EXPECT(excluded >= min_excluded, "%s: the records exclude %zu vectors for [%g, %g], expected at least %zu", name, excluded, double(lo), double(hi), min_excluded);
	// one record per vector, or the call is refused
	bool threw = false;
	try {
		std::vector<zone> fewer(zones.begin(), zones.end() - 1);
		column::select_range(blob.data(), blob.size(), PT(0), PT(1), fewer);
	} catch (const std::exception&) { threw = true; }
	EXPECT(threw, "%s: a zone map one record short did not throw", name);
	threw = false;
	try {
		column::zone_map(blob.data(), 40);
	} catch (const std::exception&) { threw = true; }
	EXPECT(threw, "%s: a blob shorter than its header did not throw", name);
	EXPECT(live_buffers == live0, "%s: %ld device buffers left allocated", name, live_buffers - live0);
	std::printf("%s: %zu values, %zu vectors, %zu excluded by the narrow band\n", name, n_values, n_vec, excluded);
}

int main() {
	run<double>("double random", random_column<double>(250 * 1024 + 333, 5), 0);
	run<float>("float random", random_column<float>(230 * 1024 + 77, 6), 0);
	run<double>("double sorted", sorted_column<double>(300 * 1024 + 100, 7), 295);
	run<float>("float sorted", sorted_column<float>(300 * 1024 + 9, 8), 295);
	std::printf("zone_test: %d failures\n", failures);
	return failures ? 1 : 0;
}
