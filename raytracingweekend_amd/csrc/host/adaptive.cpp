// adaptive.cpp — host side of rtw_adaptive.h: the active-pixel select, the
// noise estimate and the canvas with per-pixel counts, the argument checks and
// the adaptive loop's schedule (the device versions of the first three, the
// same arithmetic per pixel through moments.h, and the loop itself are in
// rtw_kernels.hip).  Plain C++, no HIP.
#include "adaptive.h"
#include <string>
#include "rtw_host_util.h"

int rtw_adaptive_check_select(const char* what, const void* accum, const void* accum_sq, const void* counts, int nx,
                              int ny, double floor, double target_rel, const void* active_out, const void* n_out) {
    const std::string w(what);
    if (!accum || !accum_sq || !counts || !active_out || !n_out) return rtw_fail(RTW_ERR_INVALID, w + ": null buffer");
    if (nx <= 0 || ny <= 0 || (uint64_t)nx * (uint64_t)ny >= (1ull << 32))
        return rtw_fail(RTW_ERR_INVALID, w + ": bad image size");
    if (!(floor > 0.0)) return rtw_fail(RTW_ERR_INVALID, w + ": floor must be positive");
    if (!(target_rel >= 0.0)) return rtw_fail(RTW_ERR_INVALID, w + ": target_rel must not be negative");
    const size_t npix = (size_t)nx * (size_t)ny;
    const struct {
        const void* p;
        size_t bytes;
    } buf[] = {{accum, npix * 24}, {accum_sq, npix * 24}, {counts, npix * 4}, {active_out, npix * 4}};
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b)
            if (rtw_spans_overlap(buf[a].p, buf[a].bytes, buf[b].p, buf[b].bytes))
                return rtw_fail(RTW_ERR_INVALID, w + ": two of the buffers overlap");
    return RTW_OK;
}

int rtw_adaptive_check_estimate(const char* what, const void* accum, const void* accum_sq, const void* counts, int nx,
                                int ny, double floor, const void* stderr_rgb) {
    // (n = 2: the per-pixel counts take its place)
    if (int rc = rtw_noise_check_args(what, accum, accum_sq, nx, ny, 2, floor, stderr_rgb)) return rc;
    const std::string w(what);
    if (!counts) return rtw_fail(RTW_ERR_INVALID, w + ": null counts");
    const size_t npix = (size_t)nx * (size_t)ny;
    if (rtw_spans_overlap(counts, npix * 4, accum, npix * 24) || rtw_spans_overlap(counts, npix * 4, accum_sq, npix * 24) ||
        (stderr_rgb && rtw_spans_overlap(counts, npix * 4, stderr_rgb, npix * 24)))
        return rtw_fail(RTW_ERR_INVALID, w + ": counts overlaps another buffer");
    return RTW_OK;
}

int rtw_adaptive_check_params(const char* what, const rtw_adaptive_params* a) {
    const std::string w(what);
    if (!a) return rtw_fail(RTW_ERR_INVALID, w + ": null adaptive parameters");
    if (!(a->target_rel >= 0.0)) return rtw_fail(RTW_ERR_INVALID, w + ": target_rel must not be negative");
    if (!(a->floor > 0.0)) return rtw_fail(RTW_ERR_INVALID, w + ": floor must be positive");
    if (a->min_spp < 2) return rtw_fail(RTW_ERR_INVALID, w + ": min_spp must be at least 2 (a variance needs two samples)");
    if (a->max_spp < a->min_spp) return rtw_fail(RTW_ERR_INVALID, w + ": max_spp must be at least min_spp");
    if (a->batch < 0) return rtw_fail(RTW_ERR_INVALID, w + ": batch must not be negative");
    return RTW_OK;
}

int rtw_adaptive_check_list(const char* what, const uint32_t* active, uint64_t n, uint64_t limit) {
    for (uint64_t k = 0; k < n; ++k) {
        if (active[k] >= limit)
            return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": pixel list entry " + std::to_string(k) + " is " +
                                                 std::to_string(active[k]) + ", the image has " + std::to_string(limit) +
                                                 " pixels");
        if (k && active[k - 1] >= active[k])
            return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": the pixel list is not strictly ascending at entry " +
                                                 std::to_string(k));
    }
    return RTW_OK;
}

extern "C" int rtw_adaptive_next_round(const rtw_adaptive_params* a, int done, int* begin, int* count) {
    if (int rc = rtw_adaptive_check_params("rtw_adaptive_next_round", a)) return rc;
    if (!begin || !count) return rtw_fail(RTW_ERR_INVALID, "rtw_adaptive_next_round: null output");
    if (done != 0 && (done < a->min_spp || done > a->max_spp))
        return rtw_fail(RTW_ERR_INVALID, "rtw_adaptive_next_round: done is 0 or in [min_spp, max_spp]");
    *begin = done;
    const int want = done == 0 ? a->min_spp : a->batch ? a->batch : done;
    const int left = a->max_spp - done;
    *count = want < left ? want : left;
    return RTW_OK;
}

extern "C" int rtw_adaptive_select(const double* accum, const double* accum_sq, const uint32_t* counts, int nx, int ny,
                                   double floor, double target_rel, uint32_t max_count, uint32_t* active_out,
                                   uint64_t* n_active_out) {
    if (int rc = rtw_adaptive_check_select("rtw_adaptive_select", accum, accum_sq, counts, nx, ny, floor, target_rel,
                                           active_out, n_active_out))
        return rc;
    const size_t npix = (size_t)nx * (size_t)ny;
    const double floor3 = 3.0 * floor;
    const rtw_count_src cnt{counts, 0};
    uint64_t n = 0;
    for (size_t p = 0; p < npix; ++p)
        if (rtw_pixel_active(accum + 3 * p, accum_sq + 3 * p, cnt[p], floor3, target_rel, max_count))
            active_out[n++] = (uint32_t)p;
    *n_active_out = n;
    return RTW_OK;
}

extern "C" int rtw_noise_estimate_counts(const double* accum, const double* accum_sq, const uint32_t* counts, int nx,
                                         int ny, double floor, double* stderr_rgb, rtw_noise_summary* out) {
    if (int rc = rtw_adaptive_check_estimate("rtw_noise_estimate_counts", accum, accum_sq, counts, nx, ny, floor,
                                             stderr_rgb))
        return rc;
    rtw_noise_estimate_pixels(accum, accum_sq, rtw_count_src{counts, 0}, (size_t)nx * (size_t)ny, floor, stderr_rgb,
                              out);
    return RTW_OK;
}

extern "C" int rtw_finalize_canvas_counts(const double* accum, const uint32_t* counts, int nx, int ny, double* canvas) {
    if (!accum || !counts || !canvas || nx <= 0 || ny <= 0)
        return rtw_fail(RTW_ERR_INVALID, "rtw_finalize_canvas_counts: bad argument");
    rtw_canvas_fill(accum, (size_t)nx * (size_t)ny * 3, rtw_div_counts{counts}, canvas);
    return RTW_OK;
}
