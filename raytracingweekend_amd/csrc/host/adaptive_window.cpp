// adaptive_window.cpp — host side of rtw_adaptive_window.h: the argument
// checks and the window select (the device select and the loop are in
// rtw_kernels.hip; both sides evaluate adaptive_window.h's predicates).  Plain
// C++, no HIP.
#include "adaptive_window.h"
#include <string>
#include <vector>
#include "rtw_host_util.h"

int rtw_adaptive_window_check_radius(const char* what, int radius) {
    if (radius < 0 || radius > RTW_WINDOW_RADIUS_MAX)
        return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": radius must lie in [0, " +
                                             std::to_string(RTW_WINDOW_RADIUS_MAX) + "]");
    return RTW_OK;
}

int rtw_adaptive_window_check_select(const char* what, const void* accum, const void* accum_sq, const void* counts,
                                     int nx, int ny, double floor, double target_rel, uint32_t min_count,
                                     uint32_t max_count, int radius, const void* active_out, const void* n_out) {
    if (int rc = rtw_adaptive_check_select(what, accum, accum_sq, counts, nx, ny, floor, target_rel, active_out, n_out))
        return rc;
    if (int rc = rtw_adaptive_window_check_radius(what, radius)) return rc;
    if (min_count > max_count)
        return rtw_fail(RTW_ERR_INVALID, std::string(what) + ": min_count must not be above max_count");
    return RTW_OK;
}

// SOURCE and "finite" once per pixel; the window through a summed-area table
// of the sources: sat[(j + 1) * (nx + 1) + (i + 1)] is the number of sources
// in rows 0..j, columns 0..i, so the number in a clipped window is four
// lookups.  (uint32_t: an image has fewer than 2^32 pixels.)
extern "C" int rtw_adaptive_select_window(const double* accum, const double* accum_sq, const uint32_t* counts, int nx,
                                          int ny, double floor, double target_rel, uint32_t min_count,
                                          uint32_t max_count, int radius, uint32_t* active_out,
                                          uint64_t* n_active_out) {
    if (int rc = rtw_adaptive_window_check_select("rtw_adaptive_select_window", accum, accum_sq, counts, nx, ny, floor,
                                                  target_rel, min_count, max_count, radius, active_out, n_active_out))
        return rc;
    const size_t npix = (size_t)nx * (size_t)ny, w = (size_t)nx + 1;
    const double floor3 = 3.0 * floor;
    std::vector<uint8_t> finite(npix);
    std::vector<uint32_t> sat(w * ((size_t)ny + 1), 0u);
    for (int j = 0; j < ny; ++j) {
        uint32_t row = 0;
        for (int i = 0; i < nx; ++i) {
            const size_t p = (size_t)j * nx + i;
            const bool fin = rtw_pixel_finite(accum + 3 * p, accum_sq + 3 * p);
            finite[p] = fin;
            row += rtw_pixel_source(accum + 3 * p, accum_sq + 3 * p, fin, counts[p], floor3, target_rel) ? 1u : 0u;
            sat[(size_t)(j + 1) * w + (i + 1)] = sat[(size_t)j * w + (i + 1)] + row;
        }
    }
    uint64_t n = 0;
    for (int j = 0; j < ny; ++j) {
        const size_t j0 = j > radius ? j - radius : 0, j1 = (size_t)(j + radius < ny - 1 ? j + radius : ny - 1) + 1;
        for (int i = 0; i < nx; ++i) {
            const size_t p = (size_t)j * nx + i;
            if (!rtw_pixel_eligible(finite[p] != 0, counts[p], min_count, max_count)) continue;
            const size_t i0 = i > radius ? i - radius : 0, i1 = (size_t)(i + radius < nx - 1 ? i + radius : nx - 1) + 1;
            const uint32_t sources = (sat[j1 * w + i1] - sat[j0 * w + i1]) - (sat[j1 * w + i0] - sat[j0 * w + i0]);
            if (sources) active_out[n++] = (uint32_t)p;
        }
    }
    *n_active_out = n;
    return RTW_OK;
}
