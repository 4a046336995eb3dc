// render_plan_check.cpp — the call plan (csrc/host/render_plan.cpp) on the CPU.
//   render_plan_check dump    one JSON line per case of render_plan_cases.h:
//                             the refusal, or every planned field and pass
//                             (tests/test_render_plan.py compares them with
//                             tests/golden/render_plan_parent.json)
//   render_plan_check check   properties no recording is needed for: the
//                             dividers, sample ids back to (i, j, s), the
//                             cameras, the staging and no-op sizes, the
//                             pools' carving, the shared sample-range check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include "host/render_plan.h"
#include "render_plan_cases.h"

static int g_bad = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                      \
            std::printf("\n");                             \
            ++g_bad;                                       \
        }                                                  \
    } while (0)

struct planned {
    int rc;
    rtw_render_params R;
    rtw_camera_desc cam;
    call_plan P;
};

static planned plan_case_call(const plan_case& c) {
    planned x;
    x.R = case_params(c);
    x.cam = case_camera(c);
    layout_facts facts;
    facts.bvh_motion = c.motion != 0, facts.shutter0 = 0.0, facts.shutter1 = 1.0;
    double* accum = reinterpret_cast<double*>(0x10000000);
    double* sq = c.moments == 0 ? nullptr : c.moments == 1 ? accum + (size_t)c.nx * c.ny * 3 : accum + 1;
    x.rc = rtw_plan_call(x.R, x.cam, facts, accum, sq, c.budget, c.strict_cus, &x.P);
    return x;
}

static std::string div_json(const rtwd::udiv32& d) {
    return "[" + std::to_string(d.m) + ", " + std::to_string(d.s1) + ", " + std::to_string(d.s2) + "]";
}

static void dump() {
    for (const plan_case& c : kPlanCases) {
        const planned x = plan_case_call(c);
        const call_plan& P = x.P;
        json_line o;
        o.str("name", c.name);
        o.i("rc", x.rc);
        if (x.rc) {
            o.str("error", rtw_last_error());
        } else if (P.noop) {
            o.u("noop", 1), o.u("samples", P.samples);
        } else {
            o.u("noop", 0);
            o.i("spp_count", P.spp_count), o.i("row_step", P.row_step), o.i("n_rows", P.n_rows), o.u("npix", P.npix);
            o.u("fast", P.fast), o.u("pin", P.pin), o.u("pool", P.pool), o.u("pass_spp", P.pass_spp);
            o.u("pass_samples", P.pass_samples);
            o.u("bytes_pool", P.bytes.pool), o.u("bytes_pool1", P.bytes.pool), o.u("bytes_fresh", P.bytes.fresh);
            o.u("bytes_hits", P.bytes.hits), o.u("bytes_radiance", P.bytes.radiance), o.u("bytes_run", P.bytes.run);
            o.u("bytes_run2", P.bytes.run2), o.u("bytes_camera", P.bytes.camera), o.u("bytes_flog", P.bytes.flog);
            o.u("hits_id_off", P.hits_id_off);
            o.u("wave_size", P.pool);
            o.raw("cam_dev", camera_bits(P.cam_dev));
            if (P.fast) o.raw("cam32", floats_bits(reinterpret_cast<const float*>(&P.cam32), 21));
            o.u("seed_mix", P.seed_mix), o.u("cam_pin", P.cam_pin), o.u("J_npix", (uint32_t)P.npix);
            o.i("J_nx", x.R.nx), o.i("J_ny", x.R.ny), o.i("J_row_begin", x.R.row_begin), o.i("J_row_step", P.row_step);
            o.i("J_max_depth", x.R.max_depth);
            o.raw("div_npix", div_json(P.div_npix)), o.raw("div_nx", div_json(P.div_nx));
            o.u("flog_threads", P.flog_threads);
            std::string passes = "[";
            for (uint64_t done = 0; done < (uint64_t)P.spp_count; done += P.pass_spp) {
                const call_pass p = rtw_plan_pass(P, x.R, done);
                passes += std::string(done ? ", " : "") + "{\"total\": " + std::to_string(p.total) +
                          ", \"spp_pass\": " + std::to_string(p.spp_pass) + ", \"div_spp\": " + div_json(p.div_spp) +
                          ", \"s_begin\": " + std::to_string(p.s_begin) + ", \"fill\": " + std::to_string(p.fill) +
                          ", \"iter_cap\": " + std::to_string(p.iter_cap) + "}";
            }
            o.raw("passes", passes + "]");
        }
        o.print();
    }
}

static bool same_div(const rtwd::udiv32& a, const rtwd::udiv32& b) { return a.m == b.m && a.s1 == b.s1 && a.s2 == b.s2; }

// sample_coords (rtw_kernels.hip) restated: pass-local id -> pixel (i, j) and
// global sample index s, by the plan's dividers
static void coords(const call_plan& P, const rtw_render_params& R, const call_pass& p, uint32_t q, int& i, int& j, int& s) {
    const uint32_t sl = rtwd::udiv_fast(q, P.div_npix);
    const uint32_t rem = q - sl * (uint32_t)P.npix;
    const uint32_t k = rtwd::udiv_fast(rem, P.div_nx);
    i = (int)(rem - k * (uint32_t)R.nx);
    j = R.row_begin + (int)k * P.row_step;
    s = p.s_begin + (int)sl;
}

static void check_job_fields(const plan_case& c, const planned& x) {
    const call_plan& P = x.P;
    CHECK(same_div(P.div_npix, rtwd::udiv_magic((uint32_t)P.npix)), "%s: div_npix", c.name);
    CHECK(same_div(P.div_nx, rtwd::udiv_magic((uint32_t)x.R.nx)), "%s: div_nx", c.name);
    uint64_t spp_seen = 0;
    for (uint64_t done = 0; done < (uint64_t)P.spp_count; done += P.pass_spp) {
        const call_pass p = rtw_plan_pass(P, x.R, done);
        CHECK(same_div(p.div_spp, rtwd::udiv_magic(p.spp_pass)), "%s: div_spp", c.name);
        CHECK((uint64_t)p.spp_pass * P.npix == p.total && (uint64_t)p.spp_pass * P.npix < (1ull << 32), "%s: total", c.name);
        CHECK(p.s_begin == x.R.spp_begin + (int)spp_seen, "%s: s_begin", c.name);
        CHECK(p.fill >= 1 && p.fill <= P.pool && p.fill <= p.total, "%s: fill", c.name);
        spp_seen += p.spp_pass;
        // the first, the last and 1 000 spread ids: sample-major, rows of the call, columns of the image
        for (int t = 0; t < 1002; ++t) {
            const uint32_t q = t == 0 ? 0 : t == 1 ? p.total - 1 : (uint32_t)(((uint64_t)p.total * (t - 2)) / 1000);
            int i, j, s;
            coords(P, x.R, p, q, i, j, s);
            const uint64_t sl = q / P.npix, rem = q % P.npix;
            const int wi = (int)(rem % x.R.nx), wj = x.R.row_begin + (int)(rem / x.R.nx) * P.row_step;
            CHECK(i == wi && j == wj && s == p.s_begin + (int)sl, "%s: id %u -> (%d, %d, %d)", c.name, q, i, j, s);
            CHECK(wj < x.R.ny && s < x.R.spp_begin + P.spp_count, "%s: id %u outside the call", c.name, q);
        }
    }
    CHECK(spp_seen == (uint64_t)P.spp_count, "%s: the passes hold %llu of %d samples per pixel", c.name,
          (unsigned long long)spp_seen, P.spp_count);
}

static void check_cameras(const plan_case& c, const planned& x) {
    const call_plan& P = x.P;
    rtw_camera_desc want = x.cam;
    if (c.camera == 1) {  // lens-less, u[1] = inf: NaN lens_radius, nothing else
        CHECK(P.cam_dev.lens_radius != P.cam_dev.lens_radius, "%s: lens_radius not NaN", c.name);
        want.lens_radius = P.cam_dev.lens_radius;
    }
    CHECK(std::memcmp(&want, &P.cam_dev, sizeof want) == 0, "%s: the device camera differs", c.name);
    CHECK(P.pin == (c.camera == 3) && P.cam_pin == (c.camera == 3 ? 1u : 0u), "%s: pinhole flag", c.name);
    if (!P.fast) return;
    const call_cam32& f = P.cam32;
    for (int k = 0; k < 3; ++k) {
        const bool ok = f.origin[k] == (float)x.cam.origin[k] && f.lower_left[k] == (float)x.cam.lower_left[k] &&
                        f.horizontal[k] == (float)x.cam.horizontal[k] && f.vertical[k] == (float)x.cam.vertical[k] &&
                        f.u[k] == (float)x.cam.u[k] && f.v[k] == (float)x.cam.v[k];
        CHECK(ok, "%s: cam32 component %d", c.name, k);
    }
    CHECK(f.time0 == (float)x.cam.time0 && f.dtime == (float)(x.cam.time1 - x.cam.time0), "%s: cam32 times", c.name);
    CHECK(f.lens_radius == (float)x.cam.lens_radius, "%s: cam32 lens_radius", c.name);  // (the caller's, never NaN)
}

struct paths_like {
    double *ox, *oy, *oz, *dx, *dy, *dz, *tm, *tr, *tg, *tb;
    uint32_t *rng, *depth, *qid;
};
struct fresh_like {
    double *ox, *oy, *oz, *dx, *dy, *dz, *tm;
    uint32_t *rng, *qid;
};
struct span {
    const char *b, *e;
    bool operator<(const span& o) const { return b < o.b; }
};
// every array inside [base, base + bytes), no two overlapping, the last one ending at base + bytes
static void check_spans(const char* what, uint32_t cap, std::set<span> s, const char* base, size_t bytes) {
    const char* at = base;
    for (const span& x : s) {
        CHECK(x.b == at && x.e > x.b, "%s cap %u: an array starts at %td, the one before ends at %td", what, cap, x.b - base,
              at - base);
        at = x.e;
    }
    CHECK(at == base + bytes, "%s cap %u: the arrays end at %td of %zu bytes", what, cap, at - base, bytes);
}
static void check_carving() {
    for (uint32_t cap : {1u, 1000u, 1u << 21}) {
        char* base = static_cast<char*>(std::malloc(rtw_paths_bytes(cap)));
        const paths_like A = rtw_carve_paths<paths_like>(base, cap);
        std::set<span> s;
        for (double* d : {A.ox, A.oy, A.oz, A.dx, A.dy, A.dz, A.tm, A.tr, A.tg, A.tb})
            s.insert({(const char*)d, (const char*)(d + cap)});
        for (uint32_t* u : {A.rng, A.depth, A.qid}) s.insert({(const char*)u, (const char*)(u + cap)});
        CHECK(s.size() == 13, "paths cap %u: arrays share a start", cap);
        check_spans("paths", cap, s, base, rtw_paths_bytes(cap));
        A.ox[0] = 1.0, A.tb[cap - 1] = 2.0, A.rng[0] = 3u, A.qid[cap - 1] = 4u;  // (the sanitizer's bounds)
        std::free(base);

        base = static_cast<char*>(std::malloc(rtw_fresh_bytes(cap)));
        const fresh_like F = rtw_carve_fresh<fresh_like>(base, cap);
        s.clear();
        for (double* d : {F.ox, F.oy, F.oz, F.dx, F.dy, F.dz, F.tm}) s.insert({(const char*)d, (const char*)(d + cap)});
        for (uint32_t* u : {F.rng, F.qid}) s.insert({(const char*)u, (const char*)(u + cap)});
        CHECK(s.size() == 9, "fresh cap %u: arrays share a start", cap);
        check_spans("fresh", cap, s, base, rtw_fresh_bytes(cap));
        F.ox[0] = 1.0, F.tm[cap - 1] = 2.0, F.rng[0] = 3u, F.qid[cap - 1] = 4u;
        std::free(base);

        // hit records: cap doubles, then cap int32
        CHECK(rtw_hits_id_off(cap) == (size_t)cap * sizeof(double) &&
                  rtw_hits_bytes(cap) == rtw_hits_id_off(cap) + (size_t)cap * sizeof(int32_t),
              "hits cap %u", cap);
    }
}

static void check_sample_range() {
    rtw_render_params R;
    std::memset(&R, 0, sizeof R);
    R.nx = R.ny = 8, R.spp = 8, R.spp_begin = 5, R.spp_count = 4;
    int n = -1;
    CHECK(rtw_check_sample_range(R, "rtw_render_multi", "rtw_render_multi: ", &n) == RTW_ERR_INVALID &&
              std::string(rtw_last_error()) == "rtw_render_multi: sample range exceeds spp",
          "multi's range text: %s", rtw_last_error());
    R.spp_count = -1;
    CHECK(rtw_check_sample_range(R, "rtw_render_multi", "rtw_render_multi: ", &n) == RTW_ERR_INVALID &&
              std::string(rtw_last_error()) == "rtw_render_multi: bad image / sample parameters",
          "multi's parameter text: %s", rtw_last_error());
    R.spp_count = 0;
    CHECK(rtw_check_sample_range(R, "rtw_render_multi", "rtw_render_multi: ", &n) == RTW_OK && n == 3, "rest of the range");
    R.spp_count = 2;
    CHECK(rtw_check_sample_range(R, "rtw_render_multi", "rtw_render_multi: ", &n) == RTW_OK && n == 2, "given count");
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "dump") {
        dump();
        return 0;
    }
    if (mode != "check") {
        std::fprintf(stderr, "usage: render_plan_check dump | check\n");
        return 2;
    }
    int planned_calls = 0;
    for (const plan_case& c : kPlanCases) {
        const planned x = plan_case_call(c);
        if (x.rc) continue;
        const call_bytes& b = x.P.bytes;
        if (x.P.noop) {  // nothing is sized
            CHECK(!b.pool && !b.fresh && !b.hits && !b.radiance && !b.run && !b.run2 && !b.camera && !b.flog && !b.staging &&
                      !x.P.pool && !x.P.pass_samples,
                  "%s: a no-op sizes a buffer", c.name);
            CHECK(x.P.samples == (uint64_t)x.P.spp_count * x.P.npix, "%s: samples", c.name);
            continue;
        }
        ++planned_calls;
        CHECK(b.staging == (c.host_accum ? (size_t)c.nx * c.ny * 24 : 0), "%s: staging bytes", c.name);
        CHECK(b.pool == rtw_paths_bytes(x.P.pool) && b.fresh == rtw_fresh_bytes(x.P.pool) &&
                  b.hits == rtw_hits_bytes(x.P.pool) && x.P.hits_id_off == rtw_hits_id_off(x.P.pool),
              "%s: pool bytes", c.name);
        CHECK(x.P.pool >= 1 && x.P.pool <= x.P.pass_samples && x.P.pass_samples <= 0xffffffffull, "%s: pool", c.name);
        check_job_fields(c, x);
        check_cameras(c, x);
    }
    check_carving();
    check_sample_range();
    if (g_bad) {
        std::printf("%d checks failed\n", g_bad);
        return 1;
    }
    std::printf("OK (%d planned calls)\n", planned_calls);
    return 0;
}
