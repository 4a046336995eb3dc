// adaptive_window.h — what the host and the device halves of
// rtw_adaptive_window.h share: the SOURCE and ELIGIBLE predicates (over
// moments.h's per-pixel expression, compiled for both sides like
// adaptive.h's rtw_pixel_active) and the argument check.
#pragma once
#include <cstddef>
#include <cstdint>
#include "adaptive.h"
#include "rtw_adaptive_window.h"

RTW_HD bool rtw_pixel_finite(const double* s1, const double* s2) {
    bool finite = true;
    for (int c = 0; c < 3; ++c) finite = finite && __builtin_isfinite(s1[c]) && __builtin_isfinite(s2[c]);
    return finite;
}

// Whether a pixel keeps its window sampling: finite moments, and either too
// few samples for a variance or rel_p > target_rel.  `finite` is
// rtw_pixel_finite of the same moments.
RTW_HD bool rtw_pixel_source(const double* s1, const double* s2, bool finite, uint32_t count, double floor3,
                             double target_rel) {
    if (!finite) return false;
    if (count < 2) return true;
    double se[3];
    bool fin;
    const double rel = rtw_pixel_rel(s1, s2, count, floor3, se, &fin);
    return rel > target_rel;
}

// Whether a pixel may be listed at all.
RTW_HD bool rtw_pixel_eligible(bool finite, uint32_t count, uint32_t min_count, uint32_t max_count) {
    return finite && count >= min_count && count < max_count;
}

// rtw_adaptive_check_select and the two arguments of the window rule.
int rtw_adaptive_window_check_select(const char* what, const void* accum, const void* accum_sq, const void* counts,
                                     int nx, int ny, double floor, double target_rel, uint32_t min_count,
                                     uint32_t max_count, int radius, const void* active_out, const void* n_out);
int rtw_adaptive_window_check_radius(const char* what, int radius);
