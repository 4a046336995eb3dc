// moments.h — the per-pixel moment statistics, once, for the host and the
// device: from a pixel's raw first / second moments and its sample count the
// mean, the clamped sample variance, the variance of the mean, the standard
// error and rel_p (rtw_noise.h's expression); the image-wide summary they add
// up to; the canvas value of a channel.  Everything compiles for both sides
// (RTW_HD, rtw_div.h), so the host loops (noise.cpp, adaptive.cpp, denoise.cpp,
// output.cpp) and the kernels of rtw_kernels.hip evaluate the same operations
// in the same order (the library builds with -ffp-contract=off).
#pragma once
#include <cstddef>
#include <cstdint>
#include "../rtw_div.h"  // (by its place: output.cpp is also built with the host directory alone on the include path)

// A pixel's sample count: counts[p], or one n for every pixel (counts null).
struct rtw_count_src {
    const uint32_t* counts;
    uint32_t n;
    RTW_HD uint32_t operator[](size_t p) const { return counts ? counts[p] : n; }
};

// The core: m[c] the mean and vm[c] the variance of the mean of each channel
// (s1 / s2 the three raw first / second moments, n the sample count).  Returns
// whether n >= 2 and the six moments are finite; n == 0 gives a NaN mean.
RTW_HD bool rtw_pixel_moments(const double* s1, const double* s2, uint32_t n, double* m, double* vm) {
    const double dn = (double)n, dn1 = dn - 1.0;
    bool fin = n >= 2;
    for (int c = 0; c < 3; ++c) {
        fin = fin && __builtin_isfinite(s1[c]) && __builtin_isfinite(s2[c]);
        m[c] = n ? s1[c] / dn : __builtin_nan("");
        double v = (s2[c] - s1[c] * m[c]) / dn1;
        if (v < 0.0) v = 0.0;
        vm[c] = v / dn;
    }
    return fin;
}

// rtw_noise.h's expression for one pixel: fills se[3], the standard error of
// each channel's mean, and returns rel_p; *finite as rtw_pixel_moments returns.
RTW_HD double rtw_pixel_rel(const double* s1, const double* s2, uint32_t n, double floor3, double* se, bool* finite) {
    double m[3];
    *finite = rtw_pixel_moments(s1, s2, n, m, se);
    for (int c = 0; c < 3; ++c) se[c] = __builtin_sqrt(se[c]);
    return ((se[0] + se[1]) + se[2]) / (((m[0] + m[1]) + m[2]) + floor3);
}

// The sums of the image-wide summary (rtw_noise_summary is rtw_noise_finish of
// them, noise.cpp): of one thread's pixels, a wave's, a block's or the image's.
struct rtw_noise_acc {
    double sum_rel, max_rel, sum_se2;
    unsigned long long pixels, nonfinite;

    static RTW_HD rtw_noise_acc empty() { return rtw_noise_acc{0.0, -__builtin_inf(), 0.0, 0, 0}; }

    // Pixel p of the estimate: accum / accum_sq the image's moments, map the
    // stderr image or null.  A pixel with fewer than two samples or a
    // non-finite moment counts in `nonfinite` and gets NaN in the map.
    RTW_HD void add_pixel(const double* accum, const double* accum_sq, const rtw_count_src& cnt, size_t p,
                          double floor3, double* map) {
        const uint32_t n = cnt[p];
        double se[3], rel = 0.0;
        bool finite = false;
        if (n >= 2) {
            const double s1[3] = {accum[3 * p], accum[3 * p + 1], accum[3 * p + 2]};
            const double s2[3] = {accum_sq[3 * p], accum_sq[3 * p + 1], accum_sq[3 * p + 2]};
            rel = rtw_pixel_rel(s1, s2, n, floor3, se, &finite);
        }
        if (!finite) {
            ++nonfinite;
            if (map) {
                const double nan = __builtin_nan("");
                map[3 * p] = nan, map[3 * p + 1] = nan, map[3 * p + 2] = nan;
            }
            return;
        }
        if (map) map[3 * p] = se[0], map[3 * p + 1] = se[1], map[3 * p + 2] = se[2];
        ++pixels;
        sum_rel = sum_rel + rel;
        if (rel > max_rel) max_rel = rel;
        sum_se2 = sum_se2 + ((se[0] * se[0] + se[1] * se[1]) + se[2] * se[2]);
    }

    RTW_HD void merge(const rtw_noise_acc& o) {
        sum_rel = sum_rel + o.sum_rel;
        sum_se2 = sum_se2 + o.sum_se2;
        if (o.max_rel > max_rel) max_rel = o.max_rel;
        pixels += o.pixels;
        nonfinite += o.nonfinite;
    }
};

// What a canvas divides a channel's sum by: one d for the image, the pixel's
// own count, or nothing (the sum is a mean already).  k indexes channels, 3 a pixel.
struct rtw_div_uniform {
    double d;
    RTW_HD double operator()(double x, size_t) const { return x / d; }
};
struct rtw_div_counts {
    const uint32_t* counts;
    RTW_HD double operator()(double x, size_t k) const { return x / (double)counts[k / 3]; }
};
struct rtw_div_none {
    RTW_HD double operator()(double x, size_t) const { return x; }
};

// canvas = min(sqrt(mean), 1) of one channel (RayTracingWeekend.cpp:241-244:
// std::min returns its first argument unless the second compares smaller, so a
// NaN passes through).
RTW_HD double rtw_canvas_value(double mean) {
    const double s = __builtin_sqrt(mean);
    return (1.0 < s) ? 1.0 : s;
}

// The host's loops.  The canvas of n channel sums over a divisor source ...
template <class D>
inline void rtw_canvas_fill(const double* sums, size_t n, D div, double* canvas) {
    for (size_t k = 0; k < n; ++k) canvas[k] = rtw_canvas_value(div(sums[k], k));
}
// ... and the estimate of npix pixels in pixel order (noise.cpp); rtw_noise_finish
// makes the summary of the image-wide sums (the device estimator's too).
struct rtw_noise_summary;
void rtw_noise_estimate_pixels(const double* accum, const double* accum_sq, const rtw_count_src& cnt, size_t npix,
                               double floor, double* stderr_rgb, rtw_noise_summary* out);
void rtw_noise_finish(const rtw_noise_acc& sums, rtw_noise_summary* out);
