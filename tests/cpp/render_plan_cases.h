// render_plan_cases.h — the calls tests/cpp/render_plan_check.cpp plans, and
// the one-line-per-case JSON both it and the recording of
// tests/golden/render_plan_parent.json print (so the two cannot drift apart
// in format).  Inputs only: no expectation lives here.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "rtw_gpu.h"

struct plan_case {
    const char* name;
    int nx, ny, spp, max_depth, spp_begin, spp_count, row_begin, row_step, wavefront_paths, precision;
    uint64_t budget;  // samples a pass may hold
    int camera;       // 0 thin lens, 1 lens-less with u[1] = inf, 2 the same with lens_radius 0.1, 3 pinhole
    int motion;       // 1: a moving-sphere BVH built for the shutter [0, 1]
    double time0, time1;
    int moments;      // 0 plain render, 1 moments with disjoint buffers, 2 with overlapping ones
    int host_accum;   // 1: the accumulators are host memory (staged)
    int strict_cus;   // the strict build's CU count (0: the product build)
};

constexpr uint64_t kDefaultBudget = 1ull << 30;

// clang-format off
static const plan_case kPlanCases[] = {
    // refusals
    {"nx_zero",          0, 8, 8, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"spp_zero",         8, 8, 0, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"begin_past_spp",   8, 8, 8, 5, 9, 0, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"count_negative",   8, 8, 8, 5, 0, -1, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"range_past_spp",   8, 8, 8, 5, 5, 4, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"precision_7",      8, 8, 8, 5, 0, 0, 0, 0, 0, 7, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"row_begin_minus1", 8, 8, 8, 5, 0, 0, -1, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"row_begin_ny",     8, 8, 8, 5, 0, 0, 8, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"image_65536",      65536, 65536, 1, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"image_46341",      46341, 46341, 1, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"shutter_outside",  8, 8, 8, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 0, 1, 0.5, 1.5, 0, 1, 0},
    {"shutter_reversed_outside", 8, 8, 8, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 0, 1, 1.0, -0.25, 0, 1, 0},
    {"moments_overlap",  8, 8, 8, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 2, 1, 0},
    // the first refusal wins
    {"nx_zero_and_precision_7", 0, 8, 8, 5, 0, 0, 0, 0, 0, 7, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"precision_7_and_row_begin_ny", 8, 8, 8, 5, 0, 0, 8, 0, 0, 7, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    // no-ops
    {"begin_equals_spp", 8, 8, 8, 5, 8, 0, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"depth_zero",       8, 8, 8, 0, 2, 3, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    // sizing
    {"passes_3_3_2",     8, 8, 16, 5, 5, 8, 0, 0, 0, 0, 192, 0, 0, 0, 1, 0, 1, 0},
    {"budget_below_npix", 8, 8, 3, 5, 0, 0, 0, 0, 0, 0, 10, 0, 0, 0, 1, 0, 1, 0},
    {"paths_default",    64, 64, 4, 50, 0, 0, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"paths_1000",       64, 64, 4, 50, 0, 0, 0, 0, 1000, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"paths_above_pass", 8, 8, 4, 50, 0, 0, 0, 0, 100000, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"rows_1_step_2",    7, 5, 4, 5, 0, 0, 1, 2, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 0},
    {"pass_cap_2_32",    4096, 4096, 1024, 50, 0, 0, 0, 0, 0, 0, 1ull << 40, 0, 0, 0, 1, 0, 0, 0},
    {"shutter_inside",   8, 8, 8, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 0, 1, 0.25, 0.75, 0, 1, 0},
    {"moments_disjoint", 8, 8, 8, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 1, 1, 0},
    {"moments_device",   8, 8, 8, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 1, 0, 0},
    {"strict_256_cus",   8, 8, 8, 7, 0, 0, 0, 0, 0, 0, kDefaultBudget, 0, 0, 0, 1, 0, 1, 256},
    // cameras, fp64 and fp32
    {"lensless_inf_u",       8, 8, 2, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 1, 0, 0, 1, 0, 1, 0},
    {"lens_inf_u",           8, 8, 2, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 2, 0, 0, 1, 0, 1, 0},
    {"pinhole",              8, 8, 2, 5, 0, 0, 0, 0, 0, 0, kDefaultBudget, 3, 0, 0, 1, 0, 1, 0},
    {"fast_thin_lens",       8, 8, 2, 5, 0, 0, 0, 0, 0, 1, kDefaultBudget, 0, 0, 0.125, 0.875, 0, 1, 0},
    {"fast_lensless_inf_u",  8, 8, 2, 5, 0, 0, 0, 0, 0, 1, kDefaultBudget, 1, 0, 0, 1, 0, 1, 0},
    {"fast_pinhole",         8, 8, 2, 5, 0, 0, 0, 0, 0, 1, kDefaultBudget, 3, 0, 0, 1, 0, 1, 0},
};
// clang-format on

inline rtw_render_params case_params(const plan_case& c) {
    rtw_render_params R;
    std::memset(&R, 0, sizeof R);
    R.nx = c.nx, R.ny = c.ny, R.spp = c.spp, R.max_depth = c.max_depth;
    R.seed = 0x123456789abcdefull + (uint64_t)c.nx;
    R.spp_begin = c.spp_begin, R.spp_count = c.spp_count, R.row_begin = c.row_begin, R.row_step = c.row_step;
    R.accum_on_device = c.host_accum ? 0 : 1;
    R.wavefront_paths = c.wavefront_paths, R.precision = c.precision;
    return R;
}

inline rtw_camera_desc case_camera(const plan_case& c) {
    rtw_camera_desc cam;
    std::memset(&cam, 0, sizeof cam);
    // values no two of which are equal, none exact in fp32
    for (int k = 0; k < 3; ++k) {
        cam.origin[k] = 1.1 + k, cam.lower_left[k] = -2.3 - 0.1 * k, cam.horizontal[k] = 4.7 + 0.01 * k;
        cam.vertical[k] = 3.3 - 0.2 * k, cam.u[k] = 0.6 + 0.03 * k, cam.v[k] = -0.7 + 0.05 * k, cam.w[k] = 0.1 * (k + 1);
    }
    cam.time0 = c.time0, cam.time1 = c.time1;
    cam.lens_radius = (c.camera == 0 || c.camera == 2) ? 0.1 : 0.0;
    if (c.camera == 1 || c.camera == 2) cam.u[1] = std::numeric_limits<double>::infinity();
    return cam;
}

// ---- printing ----------------------------------------------------------------
inline std::string hex64(double x) {
    uint64_t b;
    std::memcpy(&b, &x, 8);
    char s[32];
    std::snprintf(s, sizeof s, "\"%016llx\"", (unsigned long long)b);
    return s;
}
inline std::string hex32(float x) {
    uint32_t b;
    std::memcpy(&b, &x, 4);
    char s[16];
    std::snprintf(s, sizeof s, "\"%08x\"", b);
    return s;
}
struct json_line {
    std::string s = "{";
    void raw(const char* k, const std::string& v) { s += (s.size() > 1 ? ", \"" : "\"") + std::string(k) + "\": " + v; }
    void u(const char* k, unsigned long long v) { raw(k, std::to_string(v)); }
    void i(const char* k, long long v) { raw(k, std::to_string(v)); }
    void str(const char* k, const std::string& v) { raw(k, "\"" + v + "\""); }
    void print() { std::puts((s + "}").c_str()); }
};
// the device camera's 23 doubles / the fp32 camera's 21 floats, as bit patterns
inline std::string camera_bits(const rtw_camera_desc& c) {
    const double* d = reinterpret_cast<const double*>(&c);
    std::string s = "[";
    for (size_t k = 0; k < sizeof c / 8; ++k) s += (k ? ", " : "") + hex64(d[k]);
    return s + "]";
}
inline std::string floats_bits(const float* f, int n) {
    std::string s = "[";
    for (int k = 0; k < n; ++k) s += (k ? ", " : "") + hex32(f[k]);
    return s + "]";
}
