// denoise.cpp — host side of rtw_denoise.h: the filter on host buffers, the
// canvas step of its output and the argument checks (the device version, the
// same arithmetic per pixel through denoise.h and moments.h, and the feature
// render are in rtw_kernels.hip).  Plain C++, no HIP.
#include "denoise.h"
#include <cmath>
#include <string>
#include <utility>
#include <vector>
#include "rtw_host_util.h"

extern "C" void rtw_denoise_default_params(rtw_denoise_params* out) {
    if (!out) return;
    out->sigma_l = 4.0;
    out->sigma_z = 0.1;
    out->eps_a = 1e-2;
    out->iterations = 5;
    out->normal_power_log2 = 7;
}

int rtw_denoise_check_args(const char* what, const void* accum, const void* accum_sq, const void* counts, int n,
                           const void* features, int feature_spp, int nx, int ny, const rtw_denoise_params* p,
                           const void* out, const void* out_var) {
    const std::string w(what);
    if (!accum || !accum_sq || !features || !p || !out) return rtw_fail(RTW_ERR_INVALID, w + ": null argument");
    // (a side below 2^30: a tap's coordinate, at most 2 * 2^8 away, stays an int)
    if (nx <= 0 || ny <= 0 || nx >= (1 << 30) || ny >= (1 << 30) || (uint64_t)nx * (uint64_t)ny >= (1ull << 32))
        return rtw_fail(RTW_ERR_INVALID, w + ": bad image size");
    if (!counts && n < 2) return rtw_fail(RTW_ERR_INVALID, w + ": n must be at least 2 (a variance needs two samples)");
    if (feature_spp < 1) return rtw_fail(RTW_ERR_INVALID, w + ": feature_spp must be at least 1");
    if (p->iterations < 0 || p->iterations > 8) return rtw_fail(RTW_ERR_INVALID, w + ": iterations outside [0, 8]");
    if (p->normal_power_log2 < 0 || p->normal_power_log2 > 16)
        return rtw_fail(RTW_ERR_INVALID, w + ": normal_power_log2 outside [0, 16]");
    if (!(p->sigma_l > 0.0) || !(p->sigma_z > 0.0) || !(p->eps_a > 0.0))
        return rtw_fail(RTW_ERR_INVALID, w + ": sigma_l, sigma_z and eps_a must be positive");
    const size_t npix = (size_t)nx * (size_t)ny;
    const struct {
        const void* p;
        size_t bytes;
    } buf[] = {{out, npix * 24}, {out_var, npix * 24}, {accum, npix * 24}, {accum_sq, npix * 24},
               {counts, npix * 4}, {features, npix * 64}};
    // (the two outputs against every buffer after them; inputs may alias each other)
    for (int a = 0; a < 2; ++a)
        for (int b = a + 1; b < 6; ++b)
            if (buf[a].p && buf[b].p && rtw_spans_overlap(buf[a].p, buf[a].bytes, buf[b].p, buf[b].bytes))
                return rtw_fail(RTW_ERR_INVALID, w + ": an output overlaps another buffer");
    return RTW_OK;
}

extern "C" int rtw_denoise(const double* accum, const double* accum_sq, const uint32_t* counts, int n,
                           const double* features, int feature_spp, int nx, int ny, const rtw_denoise_params* prm,
                           double* out, double* out_var) {
    if (int rc = rtw_denoise_check_args("rtw_denoise", accum, accum_sq, counts, n, features, feature_spp, nx, ny, prm, out,
                                        out_var))
        return rc;
    const size_t npix = (size_t)nx * (size_t)ny;
    const rtw_count_src cnt{counts, (uint32_t)n};
    if (prm->iterations == 0) {
        for (size_t p = 0; p < npix; ++p) {
            double m[3], v[3];
            const bool ok = rtw_pixel_moments(accum + 3 * p, accum_sq + 3 * p, cnt[p], m, v);
            for (int c = 0; c < 3; ++c) {
                out[3 * p + c] = m[c];
                if (out_var) out_var[3 * p + c] = ok ? v[c] : std::nan("");
            }
        }
        return RTW_OK;
    }
    std::vector<rtw_dn_state> a(npix), b(npix);
    std::vector<rtw_dn_geo> geo(npix);
    std::vector<rtw_dn_alb> alb(npix);
    const double fs = (double)feature_spp;
    for (size_t p = 0; p < npix; ++p)
        rtw_dn_prepare(accum + 3 * p, accum_sq + 3 * p, cnt[p], features + 8 * p, fs, prm->eps_a, a[p], geo[p], alb[p]);
    for (int k = 0; k < prm->iterations; ++k) {
        const rtw_dn_images img{a.data(), geo.data(), alb.data(), nx};
        for (int j = 0; j < ny; ++j)
            for (int i = 0; i < nx; ++i)
                b[(size_t)j * nx + i] =
                    rtw_dn_pass(img, nx, ny, i, j, 1 << k, prm->sigma_l, prm->sigma_z, prm->normal_power_log2);
        std::swap(a, b);
    }
    for (size_t p = 0; p < npix; ++p) rtw_dn_finish(a[p], alb[p], out + 3 * p, out_var ? out_var + 3 * p : nullptr);
    return RTW_OK;
}

extern "C" int rtw_finalize_canvas_mean(const double* mean, int nx, int ny, double* canvas) {
    if (!mean || !canvas || nx <= 0 || ny <= 0) return rtw_fail(RTW_ERR_INVALID, "rtw_finalize_canvas_mean: bad argument");
    rtw_canvas_fill(mean, (size_t)nx * (size_t)ny * 3, rtw_div_none{}, canvas);
    return RTW_OK;
}
