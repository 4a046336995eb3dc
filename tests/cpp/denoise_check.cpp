// denoise_check.cpp — the host half of rtw_denoise.h (csrc/host/denoise.cpp)
// and rtw_math.h's exp_neg / pow2k in a program of its own, for a plain build
// and one under -fsanitize=address,undefined (tests/test_denoise.py).  Buffers
// are heap vectors of the exact size, so a read or write past them is a
// sanitizer report.
//   a. exp_neg against std::exp(-x): 10^5 values in [0, 50] and the cutoff's
//      neighbours within 1e-13 relative (a degree-13 Horner on |r| <= 0.35
//      truncates and rounds near 1e-15: two decades of room); 0 above the
//      cutoff and for NaN.  pow2k against repeated multiplication, exactly.
//   b. a normal edge and a coverage edge are exact: changing the colours and
//      variances of the right half leaves every left-half output bit-identical.
//   c. every documented argument error; iterations 0 returns S1/n bit for bit.
//   d. the filter on images whose last step falls off both edges (37x23, 1x1,
//      1x70, 130x5), with NaN and count-1 pixels: finite where it must be.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "denoise.h"
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

static void check_math() {
    std::mt19937_64 g(12345);
    std::uniform_real_distribution<double> u(0.0, 50.0);
    std::vector<double> xs;
    for (int k = 0; k < 100000; ++k) xs.push_back(u(g));
    const double cut = rtwd::kExpNegCutoff;
    for (double x : {0.0, 1e-300, 1e-17, 0.5 * 0.6931471805599453, std::nextafter(cut, 0.0), cut, cut - 1.0}) xs.push_back(x);
    double worst = 0.0;
    for (double x : xs) {
        const double want = std::exp(-x), got = rtwd::exp_neg(x);
        const double rel = std::fabs(got - want) / want;
        if (rel > worst) worst = rel;
    }
    std::printf("exp_neg worst relative error %.3e\n", worst);
    CHECK(worst <= 1e-13, "exp_neg: worst relative error %.3e", worst);
    CHECK(rtwd::exp_neg(0.0) == 1.0, "exp_neg(0) is 1");
    CHECK(rtwd::exp_neg(std::nextafter(cut, 1e9)) == 0.0 && rtwd::exp_neg(1e300) == 0.0 &&
              rtwd::exp_neg(std::numeric_limits<double>::infinity()) == 0.0 && rtwd::exp_neg(std::nan("")) == 0.0,
          "exp_neg is 0 above the cutoff and for NaN");
    std::uniform_real_distribution<double> v(0.0, 1.0);
    for (int k = 0; k <= 16; ++k) {
        CHECK(rtwd::pow2k(3.0, k <= 5 ? k : 5) == std::pow(3.0, 1 << (k <= 5 ? k : 5)), "pow2k(3, k) is 3^(2^k)");
        for (int t = 0; t < 100; ++t) {
            const double x = v(g);
            double y = x;
            for (int s = 0; s < k; ++s) y = y * y;
            CHECK(rtwd::pow2k(x, k) == y, "pow2k(%g, %d)", x, k);
        }
    }
    CHECK(rtwd::pow2k(0.7, 0) == 0.7 && rtwd::pow2k(0.0, 7) == 0.0 && rtwd::pow2k(1.0, 7) == 1.0, "pow2k ends");
}

struct image {
    int nx, ny, n, fs;
    std::vector<double> s1, s2, f;
    std::vector<uint32_t> counts;
};

// random moments of n samples; features: left half normal (0,0,1), right half
// `right_normal`, coverage 1 on the left and right_cov on the right
static image make_image(int nx, int ny, unsigned seed, const double* right_normal, double right_cov) {
    image im{nx, ny, 8, 4, {}, {}, {}, {}};
    const size_t npix = (size_t)nx * ny;
    im.s1.resize(npix * 3), im.s2.resize(npix * 3), im.f.resize(npix * 8), im.counts.assign(npix, 8u);
    std::mt19937_64 g(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (size_t p = 0; p < npix; ++p) {
        const bool right = (int)(p % nx) >= nx / 2;
        for (int c = 0; c < 3; ++c) {
            const double m = 0.2 + u(g), sd = 0.3 * u(g);
            im.s1[3 * p + c] = m * im.n;
            im.s2[3 * p + c] = (m * m + sd * sd) * im.n;
        }
        const double cov = right ? right_cov : 1.0;
        const double nl[3] = {0, 0, 1};
        const double* nn = right ? right_normal : nl;
        for (int c = 0; c < 3; ++c) im.f[8 * p + c] = (0.3 + 0.5 * u(g)) * im.fs;
        for (int c = 0; c < 3; ++c) im.f[8 * p + 3 + c] = nn[c] * cov * im.fs;
        im.f[8 * p + 6] = 0.25 * cov * im.fs;
        im.f[8 * p + 7] = cov * im.fs;
    }
    return im;
}

static int run(const image& im, const rtw_denoise_params& prm, bool use_counts, std::vector<double>& out,
               std::vector<double>& var) {
    out.assign(im.s1.size(), -1.0), var.assign(im.s1.size(), -1.0);
    return rtw_denoise(im.s1.data(), im.s2.data(), use_counts ? im.counts.data() : nullptr, im.n, im.f.data(), im.fs,
                       im.nx, im.ny, &prm, out.data(), var.data());
}

static void check_edges() {
    rtw_denoise_params prm;
    rtw_denoise_default_params(&prm);
    const double ortho[3] = {1, 0, 0}, same[3] = {0, 0, 1}, none[3] = {0, 0, 0};
    const struct {
        const char* name;
        const double* rn;
        double rcov;
        bool exact;
    } cases[] = {{"normal edge", ortho, 1.0, true}, {"coverage edge", none, 0.0, true}, {"no edge", same, 1.0, false}};
    for (const auto& cs : cases) {
        const int nx = 24, ny = 16;
        image a = make_image(nx, ny, 7, cs.rn, cs.rcov);
        image b = a;
        std::mt19937_64 g(99);
        std::uniform_real_distribution<double> u(0.0, 1.0);
        for (int j = 0; j < ny; ++j)
            for (int i = nx / 2; i < nx; ++i)
                for (int c = 0; c < 3; ++c) {
                    const size_t k = 3 * ((size_t)j * nx + i) + c;
                    const double m = 5.0 * u(g), sd = 2.0 * u(g);
                    b.s1[k] = m * b.n, b.s2[k] = (m * m + sd * sd) * b.n;
                }
        std::vector<double> oa, va, ob, vb;
        CHECK(run(a, prm, false, oa, va) == RTW_OK && run(b, prm, false, ob, vb) == RTW_OK, "%s: rtw_denoise", cs.name);
        bool left_same = true;
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx / 2; ++i) {
                const size_t k = 3 * ((size_t)j * nx + i);
                left_same = left_same && std::memcmp(&oa[k], &ob[k], 24) == 0 && std::memcmp(&va[k], &vb[k], 24) == 0;
            }
        // (without an edge the right half does reach the left: the test can tell)
        CHECK(left_same == cs.exact, "%s: left half %s", cs.name, left_same ? "unchanged" : "changed");
    }
}

static void check_arguments() {
    rtw_denoise_params prm;
    rtw_denoise_default_params(&prm);
    CHECK(prm.iterations == 5 && prm.sigma_l == 4.0 && prm.normal_power_log2 == 7 && prm.sigma_z == 0.1 && prm.eps_a == 1e-2,
          "the documented defaults");
    const double same[3] = {0, 0, 1};
    const image im = make_image(6, 5, 3, same, 1.0);
    std::vector<double> out(im.s1.size()), var(im.s1.size());
    const auto call = [&](const double* s1, const double* s2, const uint32_t* cn, int n, const double* f, int fs, int nx,
                          int ny, const rtw_denoise_params* p, double* o, double* v) {
        return rtw_denoise(s1, s2, cn, n, f, fs, nx, ny, p, o, v);
    };
    const double *s1 = im.s1.data(), *s2 = im.s2.data(), *f = im.f.data();
    CHECK(call(s1, s2, nullptr, 8, f, 4, 6, 5, &prm, out.data(), var.data()) == RTW_OK, "the good call");
    CHECK(call(s1, s2, nullptr, 8, f, 4, 6, 5, &prm, out.data(), nullptr) == RTW_OK, "no variance output");
    CHECK(call(nullptr, s2, nullptr, 8, f, 4, 6, 5, &prm, out.data(), nullptr) == RTW_ERR_INVALID, "null accum");
    CHECK(call(s1, nullptr, nullptr, 8, f, 4, 6, 5, &prm, out.data(), nullptr) == RTW_ERR_INVALID, "null accum_sq");
    CHECK(call(s1, s2, nullptr, 8, nullptr, 4, 6, 5, &prm, out.data(), nullptr) == RTW_ERR_INVALID, "null features");
    CHECK(call(s1, s2, nullptr, 8, f, 4, 6, 5, nullptr, out.data(), nullptr) == RTW_ERR_INVALID, "null params");
    CHECK(call(s1, s2, nullptr, 8, f, 4, 6, 5, &prm, nullptr, nullptr) == RTW_ERR_INVALID, "null output");
    CHECK(call(s1, s2, nullptr, 8, f, 4, 0, 5, &prm, out.data(), nullptr) == RTW_ERR_INVALID, "nx 0");
    CHECK(call(s1, s2, nullptr, 8, f, 4, 6, -1, &prm, out.data(), nullptr) == RTW_ERR_INVALID, "ny < 0");
    CHECK(call(s1, s2, nullptr, 1, f, 4, 6, 5, &prm, out.data(), nullptr) == RTW_ERR_INVALID, "n 1 without counts");
    CHECK(call(s1, s2, im.counts.data(), 0, f, 4, 6, 5, &prm, out.data(), nullptr) == RTW_OK, "n is not read with counts");
    CHECK(call(s1, s2, nullptr, 8, f, 0, 6, 5, &prm, out.data(), nullptr) == RTW_ERR_INVALID, "feature_spp 0");
    const double nan = std::nan("");
    for (int k = 0; k < 9; ++k) {
        rtw_denoise_params q = prm;
        if (k == 0) q.iterations = -1;
        if (k == 1) q.iterations = 9;
        if (k == 2) q.sigma_l = 0.0;
        if (k == 3) q.sigma_l = nan;
        if (k == 4) q.sigma_z = -1.0;
        if (k == 5) q.sigma_z = nan;
        if (k == 6) q.eps_a = 0.0;
        if (k == 7) q.normal_power_log2 = -1;
        if (k == 8) q.normal_power_log2 = 17;
        CHECK(call(s1, s2, nullptr, 8, f, 4, 6, 5, &q, out.data(), nullptr) == RTW_ERR_INVALID, "bad parameter %d", k);
    }
    std::vector<double> big(im.s1.size() * 2);
    CHECK(call(s1, s2, nullptr, 8, f, 4, 6, 5, &prm, big.data(), big.data() + 3) == RTW_ERR_INVALID, "out overlaps out_var");
    std::vector<double> io = im.s1;
    CHECK(call(io.data(), s2, nullptr, 8, f, 4, 6, 5, &prm, io.data(), nullptr) == RTW_ERR_INVALID, "out is accum");
    std::vector<double> fo = im.f;
    CHECK(call(s1, s2, nullptr, 8, fo.data(), 4, 6, 5, &prm, out.data(), fo.data() + 8) == RTW_ERR_INVALID,
          "out_var inside features");
    CHECK(rtw_finalize_canvas_mean(nullptr, 6, 5, out.data()) == RTW_ERR_INVALID &&
              rtw_finalize_canvas_mean(s1, 6, 0, out.data()) == RTW_ERR_INVALID, "rtw_finalize_canvas_mean's refusals");
    // iterations 0: S1 / n, bit for bit, uniform and with counts
    rtw_denoise_params z = prm;
    z.iterations = 0;
    image ic = im;
    for (size_t p = 0; p < ic.counts.size(); ++p) ic.counts[p] = 2 + (uint32_t)(p % 5);
    for (int with_counts = 0; with_counts < 2; ++with_counts) {
        CHECK(run(ic, z, with_counts != 0, out, var) == RTW_OK, "iterations 0");
        bool same_bits = true;
        for (size_t k = 0; k < out.size(); ++k) {
            const double want = ic.s1[k] / (double)(with_counts ? ic.counts[k / 3] : (uint32_t)ic.n);
            same_bits = same_bits && std::memcmp(&want, &out[k], 8) == 0;
        }
        CHECK(same_bits, "iterations 0 returns S1 / n bit for bit (counts %d)", with_counts);
    }
}

static void check_shapes() {
    rtw_denoise_params prm;
    rtw_denoise_default_params(&prm);
    const double same[3] = {0, 0, 1};
    const int sizes[][2] = {{1, 1}, {1, 70}, {37, 23}, {65, 17}, {130, 5}};
    for (const auto& sz : sizes) {
        image im = make_image(sz[0], sz[1], 11, same, 1.0);
        const size_t npix = (size_t)sz[0] * sz[1];
        const size_t pn = npix / 2, p1 = npix > 3 ? npix / 3 : 0;
        if (npix > 3) im.s1[3 * pn + 1] = std::nan(""), im.counts[p1] = 1;
        std::vector<double> out, var;
        CHECK(run(im, prm, true, out, var) == RTW_OK, "%dx%d", sz[0], sz[1]);
        for (size_t p = 0; p < npix; ++p) {
            if (npix > 3 && p == pn) {
                CHECK(std::isnan(out[3 * p + 1]) && out[3 * p] == im.s1[3 * p] / 8.0 && std::isnan(var[3 * p]),
                      "a NaN pixel passes through");
                continue;
            }
            if (npix > 3 && p == p1) {
                CHECK(out[3 * p] == im.s1[3 * p] / 1.0 && std::isnan(var[3 * p]), "a count-1 pixel passes through");
                continue;
            }
            for (int c = 0; c < 3; ++c)
                CHECK(std::isfinite(out[3 * p + c]) && out[3 * p + c] > 0.0 && std::isfinite(var[3 * p + c]) &&
                          var[3 * p + c] >= 0.0,
                      "%dx%d pixel %zu is finite", sz[0], sz[1], p);
        }
    }
}

int main() {
    check_math();
    check_edges();
    check_arguments();
    check_shapes();
    if (g_bad) {
        std::fprintf(stderr, "%d checks failed\n", g_bad);
        return 1;
    }
    std::printf("OK (denoise_check)\n");
    return 0;
}
