// adaptive_window_check.cpp — the host half of rtw_adaptive_window.h
// (csrc/host/adaptive_window.cpp) in a program of its own, for a plain build
// and one under -fsanitize=address,undefined (tests/test_adaptive_window.py).
// Buffers are heap vectors of the exact size, so a read or write past them is a
// sanitizer report.
//   a. hand-built images on quiet moments (every pixel min_count equal
//      samples): one source at each corner, at i = 63 and i = 64 of a 130-wide
//      image and in the last column lists exactly the clipped square; a NaN
//      pixel is neither listed nor a source; a pixel with one sample is a
//      source; a source at max_count is not listed but lists its neighbours;
//      a pixel below min_count is not listed.
//   b. radius 16 on a 5x3 image: one source lists every eligible pixel.
//   c. random moments (NaN / Inf pixels, counts 0, 1, 2, at and above
//      max_count) against the definition spelt out here, window by window,
//      radii 0, 1, 2 and 16; radius 0 with min_count 0 is rtw_adaptive_select.
//   d. the refusals.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "adaptive_window.h"
#include "rtw_host_util.h"

static int g_bad = 0;
#define CHECK(c, ...)                                                      \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "%s:%d: ", __FILE__, __LINE__);           \
            std::fprintf(stderr, __VA_ARGS__);                             \
            std::fputc('\n', stderr);                                      \
            ++g_bad;                                                       \
        }                                                                  \
    } while (0)

struct image {
    int nx, ny;
    std::vector<double> s1, s2;
    std::vector<uint32_t> counts;
};

// every pixel n equal samples of 0.5: variance 0, nobody a source
static image quiet(int nx, int ny, uint32_t n) {
    const size_t npix = (size_t)nx * ny;
    return image{nx, ny, std::vector<double>(npix * 3, 0.5 * n), std::vector<double>(npix * 3, 0.25 * n),
                 std::vector<uint32_t>(npix, n)};
}
static void loud(image& im, size_t p, uint32_t n = 4) {  // n samples with spread: rel ~ 0.6
    for (int c = 0; c < 3; ++c) im.s1[3 * p + c] = 1.0 * n, im.s2[3 * p + c] = 10.0 * n;
}

// the definition of rtw_adaptive_window.h, written out
static bool finite_def(const image& im, size_t p) {
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(im.s1[3 * p + c]) || !std::isfinite(im.s2[3 * p + c])) return false;
    return true;
}
static bool source_def(const image& im, size_t p, double floor, double target) {
    if (!finite_def(im, p)) return false;
    const uint32_t n = im.counts[p];
    if (n < 2) return true;
    double se[3], m[3];
    for (int c = 0; c < 3; ++c) {
        m[c] = im.s1[3 * p + c] / (double)n;
        double v = (im.s2[3 * p + c] - im.s1[3 * p + c] * m[c]) / (double)(n - 1);
        if (v < 0.0) v = 0.0;
        se[c] = std::sqrt(v / (double)n);
    }
    return ((se[0] + se[1]) + se[2]) / (((m[0] + m[1]) + m[2]) + 3.0 * floor) > target;
}
static std::vector<uint32_t> window_def(const image& im, double floor, double target, uint32_t lo, uint32_t hi, int r) {
    std::vector<uint32_t> out;
    for (int j = 0; j < im.ny; ++j)
        for (int i = 0; i < im.nx; ++i) {
            const size_t p = (size_t)j * im.nx + i;
            if (!finite_def(im, p) || im.counts[p] < lo || im.counts[p] >= hi) continue;
            bool near = false;
            for (int jj = j - r; jj <= j + r && !near; ++jj)
                for (int ii = i - r; ii <= i + r && !near; ++ii)
                    if (jj >= 0 && jj < im.ny && ii >= 0 && ii < im.nx)
                        near = source_def(im, (size_t)jj * im.nx + ii, floor, target);
            if (near) out.push_back((uint32_t)p);
        }
    return out;
}

static std::vector<uint32_t> square(const image& im, int i, int j, int r) {
    std::vector<uint32_t> out;
    for (int jj = j - r; jj <= j + r; ++jj)
        for (int ii = i - r; ii <= i + r; ++ii)
            if (jj >= 0 && jj < im.ny && ii >= 0 && ii < im.nx) out.push_back((uint32_t)(jj * im.nx + ii));
    return out;
}
static std::vector<uint32_t> without(std::vector<uint32_t> v, uint32_t p) {
    std::vector<uint32_t> out;
    for (uint32_t x : v)
        if (x != p) out.push_back(x);
    return out;
}

// the select of `im` into a list of exactly nx*ny entries; what it leaves beyond its length is checked
static std::vector<uint32_t> select(const image& im, double target, uint32_t lo, uint32_t hi, int r, const char* what) {
    const size_t npix = (size_t)im.nx * im.ny;
    std::vector<uint32_t> list(npix, 0xdeadbeefu);
    uint64_t n = ~0ull;
    const int rc = rtw_adaptive_select_window(im.s1.data(), im.s2.data(), im.counts.data(), im.nx, im.ny, 1e-2, target,
                                              lo, hi, r, list.data(), &n);
    CHECK(rc == RTW_OK, "%s: rc %d (%s)", what, rc, rtw_last_error());
    if (rc != RTW_OK || n > npix) return {};
    for (size_t k = n; k < npix; ++k)
        if (list[k] != 0xdeadbeefu) {
            CHECK(false, "%s: the select wrote past its list's end at %zu", what, k);
            break;
        }
    list.resize(n);
    CHECK(rtw_adaptive_check_list(what, list.data(), n, npix) == RTW_OK, "%s: the list is not strictly ascending", what);
    return list;
}

static void hand_cases() {
    const int nx = 130, ny = 9, r = 2;
    const uint32_t lo = 4, hi = 8;
    const double target = 0.1;
    const int spots[][3] = {{0, 0, 9}, {nx - 1, 0, 9}, {0, ny - 1, 9}, {nx - 1, ny - 1, 9}, {63, 4, 25}, {64, 4, 25},
                            {nx - 1, 4, 15}};
    for (auto& s : spots) {
        image im = quiet(nx, ny, lo);
        loud(im, (size_t)s[1] * nx + s[0]);
        const auto want = square(im, s[0], s[1], r);
        CHECK(want.size() == (size_t)s[2], "the square of (%d, %d) has %zu pixels", s[0], s[1], want.size());
        CHECK(select(im, target, lo, hi, r, "one source") == want, "one source at (%d, %d): not the clipped square", s[0], s[1]);
        CHECK(window_def(im, 1e-2, target, lo, hi, r) == want, "the definition at (%d, %d)", s[0], s[1]);
    }
    const uint32_t p = 4 * nx + 64;
    {
        image im = quiet(nx, ny, lo);
        loud(im, p);
        im.s1[3 * (p + 1) + 1] = std::nan("");
        CHECK(select(im, target, lo, hi, r, "NaN in the square") == without(square(im, 64, 4, r), p + 1),
              "a NaN pixel in the square is listed");
    }
    {
        image im = quiet(nx, ny, lo);
        im.s1[3 * p] = std::nan("");
        CHECK(select(im, target, lo, hi, r, "NaN alone").empty(), "a NaN pixel is a source");
        im = quiet(nx, ny, lo);
        im.s2[3 * p + 2] = INFINITY;
        CHECK(select(im, target, lo, hi, r, "Inf alone").empty(), "an Inf pixel is a source");
    }
    {
        image im = quiet(nx, ny, lo);
        im.counts[p] = 1;
        CHECK(select(im, target, lo, hi, r, "one sample") == without(square(im, 64, 4, r), p),
              "a pixel with one sample is a source, and below min_count not listed");
    }
    {
        image im = quiet(nx, ny, lo);
        loud(im, p, hi);
        im.counts[p] = hi;
        CHECK(select(im, target, lo, hi, r, "at max_count") == without(square(im, 64, 4, r), p),
              "a source at max_count is not listed but lists its neighbours");
    }
    {
        image im = quiet(nx, ny, lo);
        loud(im, p);
        const uint32_t q = p - nx - 2;
        im.counts[q] = lo - 1;
        for (int c = 0; c < 3; ++c) im.s1[3 * q + c] = 0.5 * (lo - 1), im.s2[3 * q + c] = 0.25 * (lo - 1);
        CHECK(select(im, target, lo, hi, r, "below min_count") == without(square(im, 64, 4, r), q),
              "a pixel below min_count inside the square is listed");
    }
    // nobody loud: an empty list, whatever the radius
    for (int rr : {0, 1, 16}) CHECK(select(quiet(nx, ny, lo), target, lo, hi, rr, "quiet").empty(), "quiet image, radius %d", rr);
}

static void radius_16_on_5x3() {
    for (size_t src = 0; src < 15; ++src) {
        image im = quiet(5, 3, 4);
        loud(im, src);
        im.counts[7] = 8;  // (the centre is at max_count: eight equal samples)
        for (int c = 0; c < 3; ++c) im.s1[3 * 7 + c] = 4.0, im.s2[3 * 7 + c] = 2.0;
        if (src == 7) loud(im, 7, 8);
        im.s1[3 * 3] = std::nan("");
        std::vector<uint32_t> want;
        for (uint32_t p = 0; p < 15; ++p)
            if (p != 7 && p != 3) want.push_back(p);
        if (src == 3) want.clear();  // (the NaN replaced the loud moments: no source at all)
        CHECK(select(im, 0.1, 4, 8, 16, "5x3 radius 16") == want, "5x3, radius 16, source %zu", src);
        CHECK(window_def(im, 1e-2, 0.1, 4, 8, 16) == want, "5x3, the definition, source %zu", src);
    }
}

static image random_image(int nx, int ny, uint32_t max_count) {
    const size_t npix = (size_t)nx * ny;
    std::mt19937_64 g(nx * 7919u + ny);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    image im{nx, ny, std::vector<double>(npix * 3, 0.0), std::vector<double>(npix * 3, 0.0), std::vector<uint32_t>(npix, 0)};
    for (size_t p = 0; p < npix; ++p) {
        const uint32_t kinds[] = {0, 1, 2, max_count - 1, max_count, max_count + 3};
        const uint32_t n = g() % 16 == 0 ? kinds[g() % 6] : 2 + (uint32_t)(g() % (max_count - 2));
        im.counts[p] = n;
        // most pixels nearly quiet, a few loud: the windows stay apart
        const double mean = 0.2 + u(g) * 2.0, spread = g() % 40 == 0 ? u(g) : 1e-3 * u(g);
        for (int c = 0; c < 3; ++c) {
            double a = 0.0, q = 0.0;
            for (uint32_t k = 0; k < n; ++k) {
                const double x = mean + spread * (u(g) - 0.5);
                a = a + x, q = q + x * x;
            }
            im.s1[3 * p + c] = a, im.s2[3 * p + c] = q;
        }
        if (g() % 97 == 0) im.s1[3 * p + g() % 3] = std::nan("");
        if (g() % 101 == 0) im.s2[3 * p + g() % 3] = INFINITY;
    }
    return im;
}

static void random_cases() {
    const int sizes[][2] = {{1, 1}, {5, 3}, {63, 4}, {64, 4}, {65, 4}, {130, 9}, {300, 7}};
    const uint32_t max_count = 64;
    const double target = 0.01;
    for (auto& sz : sizes) {
        const image im = random_image(sz[0], sz[1], max_count);
        const size_t npix = (size_t)im.nx * im.ny;
        size_t sources = 0;
        for (size_t p = 0; p < npix; ++p) sources += source_def(im, p, 1e-2, target) ? 1 : 0;
        if (npix >= 252) CHECK(sources * 100 >= npix && sources * 10 <= npix, "%dx%d: %zu sources of %zu", im.nx, im.ny, sources, npix);
        for (int r : {0, 1, 2, 16})
            for (uint32_t lo : {0u, 3u}) {
                const auto got = select(im, target, lo, max_count, r, "random");
                CHECK(got == window_def(im, 1e-2, target, lo, max_count, r), "%dx%d radius %d min_count %u: the list differs from the definition's (%zu pixels)",
                      im.nx, im.ny, r, lo, got.size());
            }
        std::vector<uint32_t> plain(npix);
        uint64_t n = 0;
        CHECK(rtw_adaptive_select(im.s1.data(), im.s2.data(), im.counts.data(), im.nx, im.ny, 1e-2, target, max_count,
                                  plain.data(), &n) == RTW_OK, "plain select");
        plain.resize(n);
        CHECK(select(im, target, 0, max_count, 0, "radius 0") == plain, "%dx%d: radius 0, min_count 0 is not rtw_adaptive_select's list", im.nx, im.ny);
    }
}

static void refusals() {
    image im = quiet(2, 2, 4);
    std::vector<uint32_t> l(4);
    uint64_t n = 0;
    const double *a = im.s1.data(), *q = im.s2.data();
    const uint32_t* c = im.counts.data();
    CHECK(rtw_adaptive_select_window(a, q, c, 2, 2, 1e-2, 0.1, 0, 8, 1, l.data(), &n) == RTW_OK && n == 0, "a valid call");
    CHECK(rtw_adaptive_select_window(a, q, c, 2, 2, 1e-2, 0.1, 8, 8, 1, l.data(), &n) == RTW_OK, "min_count == max_count");
    CHECK(rtw_adaptive_select_window(a, q, c, 2, 2, 1e-2, 0.1, 0, 8, -1, l.data(), &n) == RTW_ERR_INVALID, "radius -1");
    CHECK(rtw_adaptive_select_window(a, q, c, 2, 2, 1e-2, 0.1, 0, 8, RTW_WINDOW_RADIUS_MAX + 1, l.data(), &n) == RTW_ERR_INVALID, "radius 17");
    CHECK(rtw_adaptive_select_window(a, q, c, 2, 2, 1e-2, 0.1, 0, 8, RTW_WINDOW_RADIUS_MAX, l.data(), &n) == RTW_OK, "radius 16");
    CHECK(rtw_adaptive_select_window(a, q, c, 2, 2, 1e-2, 0.1, 9, 8, 1, l.data(), &n) == RTW_ERR_INVALID, "min_count > max_count");
    CHECK(rtw_adaptive_select_window(a, q, c, 2, 2, 0.0, 0.1, 0, 8, 1, l.data(), &n) == RTW_ERR_INVALID, "floor 0");
    CHECK(rtw_adaptive_select_window(a, q, c, 2, 2, 1e-2, -1.0, 0, 8, 1, l.data(), &n) == RTW_ERR_INVALID, "target < 0");
    CHECK(rtw_adaptive_select_window(a, q, c, 2, 2, 1e-2, std::nan(""), 0, 8, 1, l.data(), &n) == RTW_ERR_INVALID, "target NaN");
    CHECK(rtw_adaptive_select_window(a, a, c, 2, 2, 1e-2, 0.1, 0, 8, 1, l.data(), &n) == RTW_ERR_INVALID, "overlap");
    CHECK(rtw_adaptive_select_window(a, q, nullptr, 2, 2, 1e-2, 0.1, 0, 8, 1, l.data(), &n) == RTW_ERR_INVALID, "null counts");
    CHECK(rtw_adaptive_select_window(a, q, c, 2, 2, 1e-2, 0.1, 0, 8, 1, l.data(), nullptr) == RTW_ERR_INVALID, "null length");
    CHECK(rtw_adaptive_select_window(a, q, c, 0, 2, 1e-2, 0.1, 0, 8, 1, l.data(), &n) == RTW_ERR_INVALID, "nx 0");
}

int main() {
    hand_cases();
    radius_16_on_5x3();
    random_cases();
    refusals();
    if (g_bad) {
        std::fprintf(stderr, "%d checks failed\n", g_bad);
        return 1;
    }
    std::puts("OK (adaptive_window_check)");
    return 0;
}
