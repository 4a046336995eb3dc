// denoise.h — what the host and the device halves of rtw_denoise.h share: the
// filter's per-pixel and per-tap arithmetic (a pixel's mean and the variance
// of its mean: moments.h's rtw_pixel_moments) and the argument checks.  The
// functions compile for both sides (RTW_HD), so denoise.cpp's loops and the
// kernels of rtw_kernels.hip evaluate the operations rtw_denoise.h states, in
// its order (the library builds with -ffp-contract=off).
#pragma once
#include <cstddef>
#include <cstdint>
#include "moments.h"
#include "rtw_denoise.h"
#include "rtw_math.h"

// The iteration state of a pixel, 64 bytes: a tap reads it with four 16-byte
// loads.  lv < 0 marks a pixel that is not valid (c then holds its output).
struct alignas(16) rtw_dn_state {
    double c[3], l;   // demodulated mean per channel, their mean
    double v[3], lv;  // variance of c per channel, of l
};
// What stays the same across the iterations: a tap reads geo and alb.cov.
struct alignas(16) rtw_dn_geo {
    double n[3], d;  // unit normal (or 0), mean inverse depth
};
struct alignas(16) rtw_dn_alb {
    double a[3], cov;  // albedo + eps_a, coverage
};
static_assert(sizeof(rtw_dn_state) == 64 && sizeof(rtw_dn_geo) == 32 && sizeof(rtw_dn_alb) == 32, "packed for 16-byte loads");

RTW_HD void rtw_dn_set_l(rtw_dn_state& s) {
    s.l = ((s.c[0] + s.c[1]) + s.c[2]) / 3.0;
    s.lv = ((s.v[0] + s.v[1]) + s.v[2]) / 9.0;
}

// PREPARE of one pixel: f its eight feature sums, fs the feature sample count.
RTW_HD void rtw_dn_prepare(const double* s1, const double* s2, uint32_t n, const double* f, double fs, double eps_a,
                           rtw_dn_state& st, rtw_dn_geo& g, rtw_dn_alb& al) {
    double m[3], v[3];
    bool ok = rtw_pixel_moments(s1, s2, n, m, v);  // (moments.h: n < 2 is not ok, n == 0 a NaN mean)
    for (int k = 0; k < 8; ++k) ok = ok && __builtin_isfinite(f[k]);
    for (int c = 0; c < 3; ++c) {
        al.a[c] = f[c] / fs + eps_a;
        ok = ok && al.a[c] > 0.0;
        g.n[c] = f[3 + c] / fs;
    }
    g.d = f[6] / fs;
    al.cov = f[7] / fs;
    const double len = __builtin_sqrt((g.n[0] * g.n[0] + g.n[1] * g.n[1]) + g.n[2] * g.n[2]);
    if (len > 0.0)
        for (int c = 0; c < 3; ++c) g.n[c] = g.n[c] / len;
    if (!ok) {
        for (int c = 0; c < 3; ++c) st.c[c] = m[c], st.v[c] = __builtin_nan("");
        st.l = 0.0, st.lv = -1.0;
        return;
    }
    for (int c = 0; c < 3; ++c) {
        st.c[c] = m[c] / al.a[c];
        st.v[c] = v[c] / (al.a[c] * al.a[c]);
    }
    rtw_dn_set_l(st);
}

// The normal weight of a pair of pixels: cos^(2^npl2) between two non-zero
// normals, 1 between two zero ones (sky), 0 otherwise.
RTW_HD double rtw_dn_wn(const rtw_dn_geo& gp, const rtw_dn_geo& gq, int npl2) {
    const bool np = gp.n[0] != 0.0 || gp.n[1] != 0.0 || gp.n[2] != 0.0;
    const bool nq = gq.n[0] != 0.0 || gq.n[1] != 0.0 || gq.n[2] != 0.0;
    if (np && nq) {
        double dt = (gp.n[0] * gq.n[0] + gp.n[1] * gq.n[1]) + gp.n[2] * gq.n[2];
        if (!(dt > 0.0)) dt = 0.0;
        return rtwd::pow2k(dt, npl2);
    }
    return (np || nq) ? 0.0 : 1.0;
}

// Where a pass reads its input: the whole images in memory ...
struct rtw_dn_images {
    const rtw_dn_state* in;
    const rtw_dn_geo* g;
    const rtw_dn_alb* al;
    int nx;
    RTW_HD size_t at(int x, int y) const { return (size_t)y * (size_t)nx + (size_t)x; }
    RTW_HD rtw_dn_state state(int x, int y) const { return in[at(x, y)]; }
    RTW_HD double lv(int x, int y) const { return in[at(x, y)].lv; }
    RTW_HD rtw_dn_geo geo(int x, int y) const { return g[at(x, y)]; }
    RTW_HD double cov(int x, int y) const { return al[at(x, y)].cov; }
};

// One pass of one pixel (i, j).  A: rtw_dn_images, or anything that returns
// the same values for the pixels inside the image within 2 * step of (i, j)
// (the kernels' LDS tile): the arithmetic does not depend on it.
template <class A>
RTW_HD rtw_dn_state rtw_dn_pass(const A& img, int nx, int ny, int i, int j, int step, double sigma_l, double sigma_z,
                                int npl2) {
    const rtw_dn_state sp = img.state(i, j);
    if (sp.lv < 0.0) return sp;
    const rtw_dn_geo gp = img.geo(i, j);
    const double covp = img.cov(i, j);
    double gs = 0.0, gw = 0.0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int y = j + dy;
        if (y < 0 || y >= ny) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int x = i + dx;
            if (x < 0 || x >= nx) continue;
            const double lv = img.lv(x, y);
            if (lv < 0.0) continue;
            // (only neighbours a tap could read: across a geometric edge the variance does not count either)
            if (__builtin_fabs(covp - img.cov(x, y)) > 0.5 || !(rtw_dn_wn(gp, img.geo(x, y), npl2) > 0.0)) continue;
            const double wg = (double)((2 - (dy < 0 ? -dy : dy)) * (2 - (dx < 0 ? -dx : dx)));
            gs = gs + wg * lv;
            gw = gw + wg;
        }
    }
    const double den = sigma_l * __builtin_sqrt(gs / gw) + 1e-12;
    const double h[5] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
    double sw = 0.0, sc[3] = {0.0, 0.0, 0.0}, sv[3] = {0.0, 0.0, 0.0};
    for (int dy = -2; dy <= 2; ++dy) {
        const int y = j + dy * step;
        if (y < 0 || y >= ny) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int x = i + dx * step;
            if (x < 0 || x >= nx) continue;
            const rtw_dn_state sq = img.state(x, y);
            if (sq.lv < 0.0) continue;
            if (__builtin_fabs(covp - img.cov(x, y)) > 0.5) continue;
            const rtw_dn_geo gq = img.geo(x, y);
            const double wn = rtw_dn_wn(gp, gq, npl2);
            const double xl = __builtin_fabs(sp.l - sq.l) / den;
            const double xz = __builtin_fabs(gp.d - gq.d) / (sigma_z * (gp.d + gq.d) + 1e-12);
            const double w = (h[dy + 2] * h[dx + 2]) * rtwd::exp_neg(xl + xz) * wn;
            if (w > 0.0) {
                sw = sw + w;
                const double w2 = w * w;
                for (int c = 0; c < 3; ++c) {
                    sc[c] = sc[c] + w * sq.c[c];
                    sv[c] = sv[c] + w2 * sq.v[c];
                }
            }
        }
    }
    rtw_dn_state o;
    const double sw2 = sw * sw;
    for (int c = 0; c < 3; ++c) {
        o.c[c] = sc[c] / sw;
        o.v[c] = sv[c] / sw2;
    }
    rtw_dn_set_l(o);
    return o;
}

// FINISH of one pixel.
RTW_HD void rtw_dn_finish(const rtw_dn_state& s, const rtw_dn_alb& al, double* out, double* out_var) {
    const bool ok = !(s.lv < 0.0);
    for (int c = 0; c < 3; ++c) {
        out[c] = ok ? s.c[c] * al.a[c] : s.c[c];
        if (out_var) out_var[c] = ok ? s.v[c] * (al.a[c] * al.a[c]) : __builtin_nan("");
    }
}

// Argument checks shared by rtw_denoise and rtw_denoise_device (denoise.cpp);
// `what` names the entry point in the message.
int rtw_denoise_check_args(const char* what, const void* accum, const void* accum_sq, const void* counts, int n,
                           const void* features, int feature_spp, int nx, int ny, const rtw_denoise_params* p,
                           const void* out, const void* out_var);
