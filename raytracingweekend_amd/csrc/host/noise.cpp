// noise.cpp — host side of rtw_noise.h: the standard-error map of a render's
// raw moments and its image-wide summary, with one sample count or each
// pixel's own (the per-pixel arithmetic is moments.h's, which k_noise_pixels
// in rtw_kernels.hip runs too).
#include <cmath>
#include <cstdint>
#include <string>
#include "moments.h"
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

void rtw_noise_finish(const rtw_noise_acc& t, rtw_noise_summary* out) {
    out->pixels = t.pixels;
    out->nonfinite = t.nonfinite;
    out->mean_rel = t.pixels ? t.sum_rel / (double)t.pixels : 0.0;
    out->max_rel = t.pixels ? t.max_rel : 0.0;
    out->rms_stderr = t.pixels ? std::sqrt(t.sum_se2 / ((double)t.pixels * 3.0)) : 0.0;
}

void rtw_noise_estimate_pixels(const double* accum, const double* accum_sq, const rtw_count_src& cnt, size_t npix,
                               double floor, double* stderr_rgb, rtw_noise_summary* out) {
    const double floor3 = 3.0 * floor;
    rtw_noise_acc t = rtw_noise_acc::empty();
    for (size_t p = 0; p < npix; ++p) t.add_pixel(accum, accum_sq, cnt, p, floor3, stderr_rgb);
    if (out) rtw_noise_finish(t, out);
}

extern "C" int rtw_noise_estimate(const double* accum, const double* accum_sq, int nx, int ny, int n, double floor,
                                  double* stderr_rgb, rtw_noise_summary* out) {
    if (int rc = rtw_noise_check_args("rtw_noise_estimate", accum, accum_sq, nx, ny, n, floor, stderr_rgb)) return rc;
    rtw_noise_estimate_pixels(accum, accum_sq, rtw_count_src{nullptr, (uint32_t)n}, (size_t)nx * (size_t)ny, floor,
                              stderr_rgb, out);
    return RTW_OK;
}
