// noise.cpp — host side of rtw_noise.h: the standard-error map of a render's
// raw moments and its image-wide summary (the device version, the same
// arithmetic per pixel, is k_noise_pixels in rtw_kernels.hip).
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include "rtw_host_util.h"
#include "rtw_noise.h"

// [a, a+bytes) and [b, b+bytes) share a byte
bool rtw_ranges_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y ? y - x < bytes : x - y < bytes;
}

int rtw_noise_check_args(const char* what, const void* accum, const void* accum_sq, int nx, int ny, int n,
                         double floor, const void* stderr_rgb) {
    const std::string w(what);
    if (!accum || !accum_sq) return rtw_fail(RTW_ERR_INVALID, w + ": null moment buffer");
    if (nx <= 0 || ny <= 0) return rtw_fail(RTW_ERR_INVALID, w + ": bad image size");
    if (n < 2) return rtw_fail(RTW_ERR_INVALID, w + ": a variance needs n >= 2 samples per pixel");
    if (!(floor > 0.0)) return rtw_fail(RTW_ERR_INVALID, w + ": floor must be positive");
    const size_t bytes = (size_t)nx * (size_t)ny * 24;
    if (rtw_ranges_overlap(accum, accum_sq, bytes))
        return rtw_fail(RTW_ERR_INVALID, w + ": the two moment buffers overlap");
    if (stderr_rgb && (rtw_ranges_overlap(accum, stderr_rgb, bytes) || rtw_ranges_overlap(accum_sq, stderr_rgb, bytes)))
        return rtw_fail(RTW_ERR_INVALID, w + ": the stderr map overlaps a moment buffer");
    return RTW_OK;
}

void rtw_noise_finish(uint64_t pixels, uint64_t nonfinite, double sum_rel, double max_rel, double sum_se2,
                      rtw_noise_summary* out) {
    out->pixels = pixels;
    out->nonfinite = nonfinite;
    out->mean_rel = pixels ? sum_rel / (double)pixels : 0.0;
    out->max_rel = pixels ? max_rel : 0.0;
    out->rms_stderr = pixels ? std::sqrt(sum_se2 / ((double)pixels * 3.0)) : 0.0;
}

extern "C" int rtw_noise_estimate(const double* accum, const double* accum_sq, int nx, int ny, int n, double floor,
                                  double* stderr_rgb, rtw_noise_summary* out) {
    if (int rc = rtw_noise_check_args("rtw_noise_estimate", accum, accum_sq, nx, ny, n, floor, stderr_rgb)) return rc;
    const size_t npix = (size_t)nx * (size_t)ny;
    const double dn = (double)n, dn1 = (double)(n - 1), floor3 = 3.0 * floor;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    uint64_t pixels = 0, nonfinite = 0;
    double sum_rel = 0.0, max_rel = -std::numeric_limits<double>::infinity(), sum_se2 = 0.0;
    for (size_t p = 0; p < npix; ++p) {
        double se[3], m[3];
        bool finite = true;
        for (int c = 0; c < 3; ++c) {
            const double s1 = accum[3 * p + c], s2 = accum_sq[3 * p + c];
            finite = finite && std::isfinite(s1) && std::isfinite(s2);
            m[c] = s1 / dn;
            double v = (s2 - s1 * m[c]) / dn1;
            if (v < 0.0) v = 0.0;
            se[c] = std::sqrt(v / dn);
        }
        if (!finite) {
            ++nonfinite;
            if (stderr_rgb) stderr_rgb[3 * p] = stderr_rgb[3 * p + 1] = stderr_rgb[3 * p + 2] = nan;
            continue;
        }
        if (stderr_rgb) stderr_rgb[3 * p] = se[0], stderr_rgb[3 * p + 1] = se[1], stderr_rgb[3 * p + 2] = se[2];
        const double rel = ((se[0] + se[1]) + se[2]) / (((m[0] + m[1]) + m[2]) + floor3);
        ++pixels;
        sum_rel = sum_rel + rel;
        if (rel > max_rel) max_rel = rel;
        sum_se2 = sum_se2 + ((se[0] * se[0] + se[1] * se[1]) + se[2] * se[2]);
    }
    if (out) rtw_noise_finish(pixels, nonfinite, sum_rel, max_rel, sum_se2, out);
    return RTW_OK;
}
