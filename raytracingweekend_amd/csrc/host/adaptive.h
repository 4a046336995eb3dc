// adaptive.h — what the host and the device halves of rtw_adaptive.h share:
// rtw_noise.h's per-pixel expression with the pixel's own sample count, the
// active-pixel predicate, the adaptive loop's schedule and the argument
// checks.  The per-pixel functions compile for both sides (RTW_HD, rtw_div.h),
// so adaptive.cpp's loops and the kernels of rtw_kernels.hip evaluate the same
// operations in the same order (the library builds with -ffp-contract=off).
#pragma once
#include <cstddef>
#include <cstdint>
#include "rtw_adaptive.h"
#include "rtw_div.h"

// rtw_noise.h's expression for one pixel: s1 / s2 its three raw first / second
// moments, n its sample count as a double (dn1 = n - 1).  Fills se[3] and
// returns rel_p; *finite: the six moments are finite.
RTW_HD double rtw_pixel_rel(const double* s1, const double* s2, double dn, double dn1, double floor3, double* se,
                            bool* finite) {
    double m[3];
    bool fin = true;
    for (int c = 0; c < 3; ++c) {
        fin = fin && __builtin_isfinite(s1[c]) && __builtin_isfinite(s2[c]);
        m[c] = s1[c] / dn;
        double v = (s2[c] - s1[c] * m[c]) / dn1;
        if (v < 0.0) v = 0.0;
        se[c] = __builtin_sqrt(v / dn);
    }
    *finite = fin;
    return ((se[0] + se[1]) + se[2]) / (((m[0] + m[1]) + m[2]) + floor3);
}

// Whether a pixel still takes samples: fewer than max_count so far, finite
// moments, and either too few samples for a variance or rel_p > target_rel.
RTW_HD bool rtw_pixel_active(const double* s1, const double* s2, uint32_t count, double floor3, double target_rel,
                             uint32_t max_count) {
    if (count >= max_count) return false;
    bool finite = true;
    for (int c = 0; c < 3; ++c) finite = finite && __builtin_isfinite(s1[c]) && __builtin_isfinite(s2[c]);
    if (!finite) return false;
    if (count < 2) return true;
    double se[3];
    const double rel = rtw_pixel_rel(s1, s2, (double)count, (double)(count - 1), floor3, se, &finite);
    return rel > target_rel;
}

// Argument checks shared by the host and device entry points (adaptive.cpp);
// `what` names the entry point in the message.
int rtw_adaptive_check_select(const char* what, const void* accum, const void* accum_sq, const void* counts, int nx,
                              int ny, double floor, double target_rel, const void* active_out, const void* n_out);
int rtw_adaptive_check_estimate(const char* what, const void* accum, const void* accum_sq, const void* counts, int nx,
                                int ny, double floor, const void* stderr_rgb);
int rtw_adaptive_check_params(const char* what, const rtw_adaptive_params* a);
// RTW_OK when the host list is strictly ascending and below `limit`.
int rtw_adaptive_check_list(const char* what, const uint32_t* active, uint64_t n, uint64_t limit);
