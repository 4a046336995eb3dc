// adaptive_check.cpp — the host half of rtw_adaptive.h (csrc/host/adaptive.cpp)
// and the plan of an active call (csrc/host/render_plan.cpp) in a program of
// its own, for a plain build and one under -fsanitize=address,undefined
// (tests/test_adaptive.py).  Buffers are heap vectors of the exact size, so a
// read or write past them is a sanitizer report.
//   a. rtw_adaptive_select against the definition spelt out here, on random
//      moments with counts 0, 1, max_count, NaN and Inf pixels, images of
//      1x1, 300x7 and 600x500 pixels, thresholds that select none, all and
//      some; the list strictly ascending and exactly nx*ny long at most.
//   b. rtw_noise_estimate_counts and rtw_finalize_canvas_counts with uniform
//      counts against rtw_noise_estimate / rtw_finalize_canvas, bit for bit.
//   c. the list check; the schedule's rounds.
//   d. an active plan: npix == n_active, whole samples per pass, the list's
//      and counts' bytes, its refusals; a whole-image plan is unchanged by
//      the new parameter.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "adaptive.h"
#include "render_plan.h"
#include "rtw_host_util.h"

static int g_bad = 0;
#define CHECK(c, ...)                                                      \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "%s:%d: ", __FILE__, __LINE__);           \
            std::fprintf(stderr, __VA_ARGS__);                             \
            std::fputc('\n', stderr);                                      \
            ++g_bad;                                                       \
        }                                                                  \
    } while (0)

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * 8) == 0);
}

// the definition of rtw_adaptive.h, written out
static bool active_def(const double* s1, const double* s2, uint32_t n, double floor, double target, uint32_t max_count) {
    if (n >= max_count) return false;
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(s1[c]) || !std::isfinite(s2[c])) return false;
    if (n < 2) return true;
    double se[3], m[3];
    for (int c = 0; c < 3; ++c) {
        m[c] = s1[c] / (double)n;
        double v = (s2[c] - s1[c] * m[c]) / (double)(n - 1);
        if (v < 0.0) v = 0.0;
        se[c] = std::sqrt(v / (double)n);
    }
    return ((se[0] + se[1]) + se[2]) / (((m[0] + m[1]) + m[2]) + 3.0 * floor) > target;
}

static void make_moments(int nx, int ny, uint32_t max_count, std::vector<double>& s1, std::vector<double>& s2,
                         std::vector<uint32_t>& counts) {
    const size_t npix = (size_t)nx * ny;
    std::mt19937_64 g(nx * 7919u + ny);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    s1.assign(npix * 3, 0.0), s2.assign(npix * 3, 0.0), counts.assign(npix, 0);
    for (size_t p = 0; p < npix; ++p) {
        const uint32_t kinds[] = {0, 1, 2, max_count - 1, max_count, max_count + 3};
        const uint32_t n = g() % 4 == 0 ? kinds[g() % 6] : 2 + (uint32_t)(g() % (max_count - 2));
        counts[p] = n;
        const double mean = u(g) * 2.0, spread = u(g) * u(g);
        for (int c = 0; c < 3; ++c) {
            double a = 0.0, q = 0.0;
            for (uint32_t k = 0; k < n && k < 40; ++k) {
                const double x = mean + spread * (u(g) - 0.5);
                a = a + x, q = q + x * x;
            }
            s1[3 * p + c] = a, s2[3 * p + c] = q;
        }
        if (g() % 97 == 0) s1[3 * p + g() % 3] = std::nan("");
        if (g() % 101 == 0) s2[3 * p + g() % 3] = INFINITY;
    }
}

static void select_cases() {
    const int sizes[][2] = {{1, 1}, {300, 7}, {600, 500}};
    const uint32_t max_count = 64;
    for (auto& sz : sizes) {
        const int nx = sz[0], ny = sz[1];
        const size_t npix = (size_t)nx * ny;
        std::vector<double> s1, s2;
        std::vector<uint32_t> counts;
        make_moments(nx, ny, max_count, s1, s2, counts);
        for (double target : {1e9, 0.0, 0.02}) {
            std::vector<uint32_t> list(npix, 0xdeadbeefu), want;
            uint64_t n = ~0ull;
            const int rc = rtw_adaptive_select(s1.data(), s2.data(), counts.data(), nx, ny, 1e-2, target, max_count,
                                               list.data(), &n);
            CHECK(rc == RTW_OK, "select %dx%d target %g: rc %d (%s)", nx, ny, target, rc, rtw_last_error());
            for (size_t p = 0; p < npix; ++p)
                if (active_def(&s1[3 * p], &s2[3 * p], counts[p], 1e-2, target, max_count)) want.push_back((uint32_t)p);
            CHECK(n == want.size(), "select %dx%d target %g: %llu pixels, the definition %zu", nx, ny, target,
                  (unsigned long long)n, want.size());
            bool eq = n == want.size();
            for (size_t k = 0; eq && k < want.size(); ++k) eq = list[k] == want[k];
            CHECK(eq, "select %dx%d target %g: the list differs from the definition's", nx, ny, target);
            for (size_t k = want.size(); k < npix; ++k)
                if (list[k] != 0xdeadbeefu) {
                    CHECK(false, "select wrote past its list's end at %zu", k);
                    break;
                }
            CHECK(rtw_adaptive_check_list("t", list.data(), n, npix) == RTW_OK, "the list is not strictly ascending");
            if (npix > 1 && target == 0.02) CHECK(n > npix / 20 && n < npix - npix / 20, "0.02 selects %llu of %zu", (unsigned long long)n, npix);
        }
    }
    // refusals
    std::vector<double> a(12, 1.0), q(12, 1.0);
    std::vector<uint32_t> c(4, 4), l(4);
    uint64_t n = 0;
    CHECK(rtw_adaptive_select(a.data(), q.data(), c.data(), 2, 2, 0.0, 0.1, 8, l.data(), &n) == RTW_ERR_INVALID, "floor 0");
    CHECK(rtw_adaptive_select(a.data(), q.data(), c.data(), 2, 2, 1e-2, -1.0, 8, l.data(), &n) == RTW_ERR_INVALID, "target < 0");
    CHECK(rtw_adaptive_select(a.data(), q.data(), c.data(), 2, 2, 1e-2, std::nan(""), 8, l.data(), &n) == RTW_ERR_INVALID, "target NaN");
    CHECK(rtw_adaptive_select(a.data(), a.data(), c.data(), 2, 2, 1e-2, 0.1, 8, l.data(), &n) == RTW_ERR_INVALID, "overlap");
    CHECK(rtw_adaptive_select(a.data(), q.data(), c.data(), 2, 2, 1e-2, 0.1, 8, c.data(), &n) == RTW_ERR_INVALID, "list over counts");
    CHECK(rtw_adaptive_select(a.data(), q.data(), nullptr, 2, 2, 1e-2, 0.1, 8, l.data(), &n) == RTW_ERR_INVALID, "null counts");
    CHECK(rtw_adaptive_select(a.data(), q.data(), c.data(), 0, 2, 1e-2, 0.1, 8, l.data(), &n) == RTW_ERR_INVALID, "nx 0");
}

static void uniform_cases() {
    const int nx = 37, ny = 11;
    const size_t npix = (size_t)nx * ny;
    std::vector<double> s1, s2;
    std::vector<uint32_t> counts;
    make_moments(nx, ny, 64, s1, s2, counts);
    for (int n : {2, 7, 64}) {
        std::vector<uint32_t> uni(npix, (uint32_t)n);
        std::vector<double> se_a(npix * 3), se_b(npix * 3), cv_a(npix * 3), cv_b(npix * 3);
        rtw_noise_summary A, B;
        CHECK(rtw_noise_estimate(s1.data(), s2.data(), nx, ny, n, 1e-2, se_a.data(), &A) == RTW_OK, "estimate");
        CHECK(rtw_noise_estimate_counts(s1.data(), s2.data(), uni.data(), nx, ny, 1e-2, se_b.data(), &B) == RTW_OK,
              "estimate_counts: %s", rtw_last_error());
        CHECK(same_bits(se_a, se_b), "n %d: the map with uniform counts differs from rtw_noise_estimate's", n);
        CHECK(std::memcmp(&A, &B, sizeof A) == 0, "n %d: the summary with uniform counts differs", n);
        rtw_finalize_canvas(s1.data(), nx, ny, n, cv_a.data());
        CHECK(rtw_finalize_canvas_counts(s1.data(), uni.data(), nx, ny, cv_b.data()) == RTW_OK, "finalize_counts");
        CHECK(same_bits(cv_a, cv_b), "n %d: the canvas with uniform counts differs from rtw_finalize_canvas's", n);
    }
    // mixed counts: pixels below two samples are left out, NaN in the map
    std::vector<double> se(npix * 3);
    rtw_noise_summary S;
    CHECK(rtw_noise_estimate_counts(s1.data(), s2.data(), counts.data(), nx, ny, 1e-2, se.data(), &S) == RTW_OK, "mixed");
    uint64_t out = 0;
    for (size_t p = 0; p < npix; ++p) {
        bool fin = counts[p] >= 2;
        for (int c = 0; c < 3; ++c) fin = fin && std::isfinite(s1[3 * p + c]) && std::isfinite(s2[3 * p + c]);
        out += fin ? 0 : 1;
        CHECK(std::isnan(se[3 * p]) == !fin, "pixel %zu: NaN in the map iff left out", p);
    }
    CHECK(S.nonfinite == out && S.pixels == npix - out && out > 0, "mixed counts: %llu left out, expected %llu",
          (unsigned long long)S.nonfinite, (unsigned long long)out);
    CHECK(rtw_noise_estimate_counts(s1.data(), s2.data(), nullptr, nx, ny, 1e-2, nullptr, &S) == RTW_ERR_INVALID, "null counts");
    CHECK(rtw_finalize_canvas_counts(s1.data(), nullptr, nx, ny, se.data()) == RTW_ERR_INVALID, "null counts");
}

static void list_and_schedule() {
    const uint32_t ok[] = {0, 1, 5, 99}, dup[] = {0, 5, 5, 9}, down[] = {3, 2}, far[] = {0, 100};
    CHECK(rtw_adaptive_check_list("t", ok, 4, 100) == RTW_OK, "ascending list refused");
    CHECK(rtw_adaptive_check_list("t", ok, 0, 100) == RTW_OK, "empty list refused");
    CHECK(rtw_adaptive_check_list("t", dup, 4, 100) == RTW_ERR_INVALID, "duplicate accepted");
    CHECK(rtw_adaptive_check_list("t", down, 2, 100) == RTW_ERR_INVALID, "descending accepted");
    CHECK(rtw_adaptive_check_list("t", far, 2, 100) == RTW_ERR_INVALID, "out of range accepted");
    struct {
        int min_spp, max_spp, batch;
        std::vector<std::pair<int, int>> want;
    } cases[] = {{8, 32, 8, {{0, 8}, {8, 8}, {16, 8}, {24, 8}}},
                 {8, 50, 0, {{0, 8}, {8, 8}, {16, 16}, {32, 18}}},
                 {16, 16, 0, {{0, 16}}},
                 {2, 9, 4, {{0, 2}, {2, 4}, {6, 3}}},
                 {4, 1024, 0, {{0, 4}, {4, 4}, {8, 8}, {16, 16}, {32, 32}, {64, 64}, {128, 128}, {256, 256}, {512, 512}}}};
    for (auto& c : cases) {
        rtw_adaptive_params ap;
        std::memset(&ap, 0, sizeof ap);
        ap.target_rel = 0.1, ap.floor = 1e-2, ap.min_spp = c.min_spp, ap.max_spp = c.max_spp, ap.batch = c.batch;
        int done = 0;
        std::vector<std::pair<int, int>> got;
        for (;;) {
            int b = -1, n = -1;
            CHECK(rtw_adaptive_next_round(&ap, done, &b, &n) == RTW_OK, "next_round: %s", rtw_last_error());
            if (n <= 0) break;
            got.push_back({b, n});
            done = b + n;
        }
        CHECK(got == c.want && done == c.max_spp, "schedule min %d max %d batch %d: %zu rounds, done %d", c.min_spp,
              c.max_spp, c.batch, got.size(), done);
    }
    rtw_adaptive_params bad;
    std::memset(&bad, 0, sizeof bad);
    bad.target_rel = 0.1, bad.floor = 1e-2, bad.min_spp = 1, bad.max_spp = 8;
    int b, n;
    CHECK(rtw_adaptive_next_round(&bad, 0, &b, &n) == RTW_ERR_INVALID, "min_spp 1");
    bad.min_spp = 9;
    CHECK(rtw_adaptive_next_round(&bad, 0, &b, &n) == RTW_ERR_INVALID, "max_spp < min_spp");
    bad.min_spp = 4, bad.batch = -1;
    CHECK(rtw_adaptive_next_round(&bad, 0, &b, &n) == RTW_ERR_INVALID, "batch < 0");
    bad.batch = 0, bad.floor = 0.0;
    CHECK(rtw_adaptive_next_round(&bad, 0, &b, &n) == RTW_ERR_INVALID, "floor 0");
    bad.floor = 1e-2;
    CHECK(rtw_adaptive_next_round(&bad, 3, &b, &n) == RTW_ERR_INVALID, "done below min_spp");
    CHECK(rtw_adaptive_next_round(&bad, 9, &b, &n) == RTW_ERR_INVALID, "done above max_spp");
    CHECK(rtw_adaptive_next_round(nullptr, 0, &b, &n) == RTW_ERR_INVALID, "null params");
}

static void plan_cases() {
    rtw_render_params R;
    std::memset(&R, 0, sizeof R);
    R.nx = 64, R.ny = 48, R.spp = 16, R.max_depth = 50, R.seed = 7, R.spp_begin = 3, R.spp_count = 8, R.row_step = 1;
    rtw_camera_desc cam;
    std::memset(&cam, 0, sizeof cam);
    cam.origin[0] = cam.origin[1] = cam.origin[2] = 1.0;
    layout_facts facts{};
    std::vector<double> accum(64 * 48 * 3), sq(64 * 48 * 3);
    std::vector<uint32_t> counts(64 * 48), list(1025);
    const call_active act{1025, list.data(), counts.data()};
    call_plan whole, whole2, P;
    CHECK(rtw_plan_call(R, cam, facts, accum.data(), sq.data(), 3 * 1025, 0, &P, &act) == RTW_OK, "active plan: %s",
          rtw_last_error());
    CHECK(P.active && P.npix == 1025 && P.pass_spp == 3 && P.pass_samples == 3 * 1025, "npix %llu pass_spp %llu",
          (unsigned long long)P.npix, (unsigned long long)P.pass_spp);
    CHECK(P.bytes.run == 1025 * 24 && P.bytes.run2 == 1025 * 24 && P.bytes.radiance == 3 * 1025 * 24, "per-pixel bytes");
    CHECK(P.bytes.list == 1025 * 4 && P.bytes.counts == 64 * 48 * 4 && P.bytes.staging == 64 * 48 * 24, "list / counts bytes");
    CHECK(P.div_npix.m == rtwd::udiv_magic(1025).m, "div_npix is the list length's");
    int spp[3], k = 0;
    for (uint64_t done = 0; done < (uint64_t)P.spp_count; done += P.pass_spp) {
        const call_pass p = rtw_plan_pass(P, R, done);
        CHECK(p.total == p.spp_pass * 1025, "a pass holds whole samples of every listed pixel");
        if (k < 3) spp[k] = (int)p.spp_pass;
        ++k;
    }
    CHECK(k == 3 && spp[0] == 3 && spp[1] == 3 && spp[2] == 2, "passes 3 + 3 + 2");
    R.accum_on_device = 1;
    CHECK(rtw_plan_call(R, cam, facts, accum.data(), sq.data(), 1 << 20, 0, &P, &act) == RTW_OK, "device plan");
    CHECK(P.bytes.list == 0 && P.bytes.counts == 0 && P.bytes.staging == 0, "device buffers need no copies");
    R.accum_on_device = 0;
    // a whole-image plan does not change with the new parameter's default
    CHECK(rtw_plan_call(R, cam, facts, accum.data(), sq.data(), 1 << 20, 0, &whole) == RTW_OK, "whole");
    CHECK(rtw_plan_call(R, cam, facts, accum.data(), sq.data(), 1 << 20, 0, &whole2, nullptr) == RTW_OK, "whole");
    CHECK(!whole.active && whole.npix == 64 * 48 && whole.bytes.list == 0 && whole.bytes.counts == 0 &&
              whole.npix == whole2.npix && whole.pass_spp == whole2.pass_spp, "the whole-image plan");
    // an empty list: a no-op of no samples
    const call_active none{0, nullptr, counts.data()};
    CHECK(rtw_plan_call(R, cam, facts, accum.data(), sq.data(), 1 << 20, 0, &P, &none) == RTW_OK && P.noop && P.samples == 0,
          "empty list");
    // refusals
    rtw_render_params Q = R;
    Q.row_begin = 1;
    CHECK(rtw_plan_call(Q, cam, facts, accum.data(), sq.data(), 1 << 20, 0, &P, &act) == RTW_ERR_INVALID, "row_begin 1");
    Q = R, Q.row_step = 2;
    CHECK(rtw_plan_call(Q, cam, facts, accum.data(), sq.data(), 1 << 20, 0, &P, &act) == RTW_ERR_INVALID, "row_step 2");
    Q = R, Q.row_step = 0;
    CHECK(rtw_plan_call(Q, cam, facts, accum.data(), sq.data(), 1 << 20, 0, &P, &act) == RTW_OK, "row_step 0 means 1");
    const call_active many{64 * 48 + 1, list.data(), nullptr}, null_list{5, nullptr, nullptr};
    CHECK(rtw_plan_call(R, cam, facts, accum.data(), sq.data(), 1 << 20, 0, &P, &many) == RTW_ERR_INVALID, "too many pixels");
    CHECK(rtw_plan_call(R, cam, facts, accum.data(), sq.data(), 1 << 20, 0, &P, &null_list) == RTW_ERR_INVALID, "null list");
    const call_active over{16, reinterpret_cast<const uint32_t*>(accum.data() + 6), nullptr};
    CHECK(rtw_plan_call(R, cam, facts, accum.data(), sq.data(), 1 << 20, 0, &P, &over) == RTW_ERR_INVALID, "list in accum");
    const call_active cover{16, list.data(), reinterpret_cast<uint32_t*>(sq.data())};
    CHECK(rtw_plan_call(R, cam, facts, accum.data(), sq.data(), 1 << 20, 0, &P, &cover) == RTW_ERR_INVALID, "counts in accum_sq");
    const call_active lc{16, counts.data() + 8, counts.data()};
    CHECK(rtw_plan_call(R, cam, facts, accum.data(), nullptr, 1 << 20, 0, &P, &lc) == RTW_ERR_INVALID, "list in counts");
}

int main() {
    select_cases();
    uniform_cases();
    list_and_schedule();
    plan_cases();
    if (g_bad) {
        std::fprintf(stderr, "%d checks failed\n", g_bad);
        return 1;
    }
    std::puts("OK (adaptive_check)");
    return 0;
}
