// adaptive.h — what the host and the device halves of rtw_adaptive.h share:
// the active-pixel predicate (over moments.h's per-pixel expression, compiled
// for both sides like it), the adaptive loop's schedule and the argument
// checks.
#pragma once
#include <cstddef>
#include <cstdint>
#include "moments.h"
#include "rtw_adaptive.h"

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
    const double rel = rtw_pixel_rel(s1, s2, count, floor3, se, &finite);
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
