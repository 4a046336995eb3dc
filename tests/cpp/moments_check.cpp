// moments_check.cpp — csrc/host/moments.h alone on its edge pixels: the core
// with n of 0, 1 and 2, NaN and inf moments and a negative variance, the
// summary's add and merge (an image of non-finite pixels among them), the count
// and divisor sources and the canvas value.  A program of its own, built with
// g++ -fsanitize=address,undefined by tests/test_moment_stats.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "moments.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static const double kNan = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

static const double kRel = 3.0 / (6.0 + 0.03);  // se 1 + 1 + 1 over mean 2 + 2 + 2 and 3 * floor

static bool same(const rtw_noise_acc& a, const rtw_noise_acc& b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main() {
    double m[3], v[3], se[3];
    bool fin;
    // two samples 1 and 3 per channel: mean 2, variance 2, variance of the mean 1
    const double s1[3] = {4, 4, 4}, s2[3] = {10, 10, 10};
    CHECK(rtw_pixel_moments(s1, s2, 2, m, v) && m[0] == 2 && v[2] == 1);
    CHECK(rtw_pixel_rel(s1, s2, 2, 0.03, se, &fin) == kRel && fin && se[1] == 1);
    // no sample: a NaN mean; one: the mean, no variance; neither is ok
    CHECK(!rtw_pixel_moments(s1, s2, 0, m, v) && std::isnan(m[0]) && std::isnan(v[0]));
    CHECK(!rtw_pixel_moments(s1, s2, 1, m, v) && m[1] == 4 && v[1] == 0);  // (-6 / 0 clamps like any negative)
    // a variance below zero (rounding, or moments that belong to no samples) is 0
    const double low[3] = {7, 7, 7};
    CHECK(rtw_pixel_moments(s1, low, 2, m, v) && v[0] == 0 && v[1] == 0 && v[2] == 0);
    CHECK(rtw_pixel_rel(s1, low, 2, 0.03, se, &fin) == 0 && fin);
    // NaN and inf moments
    const double n1[3] = {4, kNan, 4}, i2[3] = {kInf, 10, 10};
    CHECK(!rtw_pixel_moments(n1, s2, 2, m, v) && std::isnan(m[1]) && m[0] == 2);
    CHECK(!rtw_pixel_moments(s1, i2, 2, m, v) && v[0] == kInf && v[1] == 1);

    // the summary: pixels 0 and 3 count, 1 (NaN), 2 (inf) and 4 (one sample) do not
    const uint32_t npix = 5;
    std::vector<double> a, q, map(3 * npix, -1.0);
    const double* const p1[npix] = {s1, n1, s1, s1, s1};
    const double* const p2[npix] = {s2, s2, i2, low, s2};
    for (uint32_t p = 0; p < npix; ++p) a.insert(a.end(), p1[p], p1[p] + 3), q.insert(q.end(), p2[p], p2[p] + 3);
    const std::vector<uint32_t> counts = {2, 2, 2, 2, 1};
    const rtw_count_src per_pixel{counts.data(), 0}, uniform{nullptr, 2};
    CHECK(per_pixel[4] == 1 && uniform[4] == 2);
    rtw_noise_acc t = rtw_noise_acc::empty(), left = t, right = t;
    for (uint32_t p = 0; p < npix; ++p) {
        t.add_pixel(a.data(), q.data(), per_pixel, p, 0.03, map.data());
        (p < 2 ? left : right).add_pixel(a.data(), q.data(), per_pixel, p, 0.03, nullptr);
    }
    CHECK(t.pixels == 2 && t.nonfinite == 3 && t.sum_rel == kRel && t.max_rel == kRel && t.sum_se2 == 3);
    CHECK(map[0] == 1 && std::isnan(map[3]) && std::isnan(map[8]) && map[9] == 0 && std::isnan(map[14]));
    left.merge(right);
    CHECK(same(left, t));
    // with one n for every pixel the last pixel counts too
    rtw_noise_acc u = rtw_noise_acc::empty();
    for (uint32_t p = 0; p < npix; ++p) u.add_pixel(a.data(), q.data(), uniform, p, 0.03, nullptr);
    CHECK(u.pixels == 3 && u.nonfinite == 2 && u.sum_se2 == 6);
    // an image of non-finite pixels: nothing but the counter moves, and a merge keeps that
    rtw_noise_acc none = rtw_noise_acc::empty(), e = rtw_noise_acc::empty();
    for (int k = 0; k < 3; ++k) none.add_pixel(a.data(), q.data(), uniform, 1, 0.03, map.data());
    CHECK(none.pixels == 0 && none.nonfinite == 3 && none.sum_rel == 0 && none.max_rel == -kInf && none.sum_se2 == 0);
    e.merge(none);
    CHECK(same(e, none));
    none.merge(t);
    CHECK(none.pixels == 2 && none.nonfinite == 6 && none.max_rel == t.max_rel);

    // the canvas value and the divisor sources
    CHECK(rtw_canvas_value(0.25) == 0.5 && rtw_canvas_value(4) == 1 && rtw_canvas_value(kInf) == 1);
    CHECK(std::isnan(rtw_canvas_value(kNan)) && std::isnan(rtw_canvas_value(-1)) && rtw_canvas_value(0) == 0);
    CHECK(rtw_div_uniform{4}(1, 7) == 0.25 && rtw_div_counts{counts.data()}(1, 14) == 1 && rtw_div_none{}(3, 0) == 3);
    CHECK(rtw_div_counts{counts.data()}(1, 11) == 0.5 && std::isnan(rtw_div_uniform{0}(0, 0)));
    double canvas[15];
    rtw_canvas_fill(a.data(), 15, rtw_div_counts{counts.data()}, canvas);
    CHECK(canvas[0] == 1 && std::isnan(canvas[4]) && canvas[12] == 1);
    rtw_canvas_fill(map.data(), 15, rtw_div_none{}, canvas);
    CHECK(canvas[0] == 1 && std::isnan(canvas[3]) && canvas[9] == 0);
    std::printf("OK (moments_check)\n");
    return 0;
}
