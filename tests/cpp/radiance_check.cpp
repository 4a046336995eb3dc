// radiance_check.cpp — csrc/host/radiance.cpp and rtw_select.h's select_rays on
// the CPU: every refusal of rtw_radiance_check_args, rtw_radiance_plan's chunks
// and passes (the chunks tile [0, n) exactly once with first_key offsets that
// add up, no pass above the 32-bit sample id or the budget, staged chunks within
// the byte bound), and the ray-sourced kernel choice over select_check.cpp's
// grid.  Prints rtw_radiance_params' size and offsets for tests/test_radiance.py,
// the built-in scenes' choices, then "OK (radiance_check)".
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "radiance.h"
#include "rtw_host_util.h"
#include "rtw_select.h"

using namespace rtwd;

namespace {
int fails = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            ++fails;                                                 \
        }                                                            \
    } while (0)

rtw_radiance_params params(int depth, int begin, int count, bool dev, uint32_t key = 0) {
    rtw_radiance_params p;
    std::memset(&p, 0, sizeof p);
    p.max_depth = depth, p.spp_begin = begin, p.spp_count = count, p.on_device = dev, p.first_key = key;
    p.seed = 99, p.precision = RTW_PRECISION_FP64;
    return p;
}

// The chunks and passes of one plan; walks at most `walk` chunks from either end
// (a plan of 2^32 - 1 rays under a small bound has millions).
void plan_case(uint64_t n, const rtw_radiance_params& p, bool with_rng, size_t budget, size_t stage_bytes,
               uint64_t chunk_max, uint64_t walk = 64) {
    const radiance_plan P = rtw_radiance_plan(n, p, with_rng, budget, stage_bytes, chunk_max);
    CHECK(P.n == n && P.staged == !p.on_device && P.samples == n * (uint64_t)p.spp_count);
    if (n == 0 || p.max_depth == 0) {
        CHECK(P.noop && P.n_chunks == 0);
        std::printf("plan n=%llu spp=%d staged=%d: no-op\n", (unsigned long long)n, p.spp_count, (int)P.staged);
        return;
    }
    CHECK(!P.noop && P.n_chunks >= 1 && P.chunk_rays >= 1);
    CHECK((P.n_chunks - 1) * P.chunk_rays < n && P.n_chunks * P.chunk_rays >= n);  // the chunks tile [0, n)
    CHECK(P.chunk_rays <= kRadianceChunkMax && P.chunk_rays <= chunk_max && (P.chunk_rays <= budget || P.chunk_rays == 1));
    const size_t ray_bytes = 64 + 24 + (with_rng ? 4 : 0);
    if (P.staged) {
        CHECK(P.chunk_rays * ray_bytes <= stage_bytes || P.chunk_rays == 1);
        CHECK(P.bytes_rays == P.chunk_rays * 64 && P.bytes_sums == P.chunk_rays * 24);
        CHECK(P.bytes_rng == (with_rng ? P.chunk_rays * 4 : 0));
    } else {
        CHECK(P.bytes_rays == 0 && P.bytes_sums == 0 && P.bytes_rng == 0);
    }
    uint64_t passes = 0;
    for (uint64_t c = 0; c < P.n_chunks; ++c) {
        if (c >= walk && c + walk < P.n_chunks) continue;
        radiance_chunk ch;
        CHECK(rtw_radiance_chunk(P, c, &ch) == RTW_OK);
        CHECK(ch.first == c * P.chunk_rays && ch.count >= 1 && ch.first + ch.count <= n);
        CHECK(c + 1 < P.n_chunks ? ch.count == P.chunk_rays : ch.first + ch.count == n);
        CHECK((uint64_t)ch.first_key == (uint64_t)p.first_key + ch.first);  // (never wraps: first_key + n <= 2^32)
        const call_plan& C = ch.call;
        CHECK(!C.noop && !C.fast && !C.active && C.npix == ch.count && C.spp_count == p.spp_count);
        CHECK(C.pass_spp >= 1 && C.pass_samples == C.pass_spp * ch.count && C.pass_samples <= 0xffffffffull);
        CHECK(C.pass_samples <= budget || C.pass_spp == 1);
        CHECK(C.bytes.radiance == C.pass_samples * 24 && C.bytes.run == ch.count * 24 && C.bytes.staging == 0);
        CHECK(C.pool >= 1 && C.pool <= C.pass_samples);
        CHECK(C.seed_mix == rtw_splitmix64(p.seed));
        uint64_t done = 0;
        int s_next = p.spp_begin;
        for (; done < (uint64_t)C.spp_count; done += C.pass_spp, ++passes) {
            const call_pass pass = rtw_plan_pass(C, ch.R, done);
            CHECK(pass.s_begin == s_next && pass.spp_pass >= 1 && pass.total == pass.spp_pass * ch.count);
            CHECK(pass.fill >= 1 && pass.fill <= C.pool);
            s_next += (int)pass.spp_pass;
        }
        CHECK(s_next == p.spp_begin + p.spp_count);
    }
    std::printf("plan n=%llu spp=%d staged=%d rng=%d: %llu chunks of %llu, %llu passes walked\n", (unsigned long long)n,
                p.spp_count, (int)P.staged, (int)with_rng, (unsigned long long)P.n_chunks,
                (unsigned long long)P.chunk_rays, (unsigned long long)passes);
}

// ---- select_rays ---------------------------------------------------------------------
std::map<std::string, long> g_kinds;

void check_rays(const select_in& s) {
    const kernel_choice c = select_rays(s);
    CHECK(c.rays && !c.active);
    CHECK(!(c.id.f & F_PIN) && !(c.id.f & F_ACTIVE));
    // what a render through a camera that is no pinhole runs
    select_in r = s;
    r.active = false, r.pin = false;
    const kernel_choice whole = select_fp64(r);
    if (c.persistent()) {
        CHECK(index_of(kPersistRaysList, active_inst{c.id, c.form}) >= 0);
        CHECK((c.id.f & F_RAYS) && (c.id.f & ~F_RAYS) == whole.id.f && c.id.m == whole.id.m && c.id.l == whole.id.l &&
              c.form == whole.form);
        CHECK(!s.strict && !s.env.wavefront);
        ++g_kinds["persistent row"];
        return;
    }
    r.env.wavefront = true;
    const kernel_choice want = select_fp64(r);
    CHECK(c.form == want.form && c.id == want.id && c.name == "k_regen_rays + " + want.name);
    CHECK(!(c.id.f & F_RAYS));
    if (c.form == kform::segment) {
        CHECK(index_of(kSegmentList, c.id) >= 0);
        ++g_kinds["k_regen_rays + k_segment"];
    } else {
        const split_rows rows = split_resolve(c.id);
        CHECK(index_of(kIntersectList, rows.intersect) >= 0 && index_of(kShadeList, rows.shade) >= 0);
        ++g_kinds["k_regen_rays + split pair"];
    }
    // the parent's choices do not read the new field
    select_in a = s;
    a.active = false;
    const kernel_choice plain = select_fp64(a);
    CHECK(!plain.rays);
}
}  // namespace

int main() {
    std::printf("sizeof rtw_radiance_params %zu max_depth %zu spp_begin %zu spp_count %zu on_device %zu seed %zu "
                "first_key %zu precision %zu wavefront_paths %zu pad %zu\n",
                sizeof(rtw_radiance_params), offsetof(rtw_radiance_params, max_depth),
                offsetof(rtw_radiance_params, spp_begin), offsetof(rtw_radiance_params, spp_count),
                offsetof(rtw_radiance_params, on_device), offsetof(rtw_radiance_params, seed),
                offsetof(rtw_radiance_params, first_key), offsetof(rtw_radiance_params, precision),
                offsetof(rtw_radiance_params, wavefront_paths), offsetof(rtw_radiance_params, pad));

    // ---- rtw_radiance_check_args ------------------------------------------------------
    alignas(64) static char buf[4096];
    int handle = 0;
    const void* h = &handle;
    const void* rays = buf;         // 8 rays: 512 bytes
    const void* sums = buf + 1024;  // 8 x 24 bytes
    const void* rng = buf + 2048;   // 8 states
    const uint64_t n = 8;
    const rtw_radiance_params host = params(50, 2, 3, false), dev = params(50, 2, 3, true);
    const rtw_radiance_params host1 = params(50, 0, 1, false), dev1 = params(50, 0, 1, true);
    auto check = [&](const void* hh, const void* r, uint64_t m, const void* g, const rtw_radiance_params* p, const void* s,
                     bool strict = false) { return rtw_radiance_check_args(hh, r, m, g, p, s, strict); };
    CHECK(check(h, rays, n, nullptr, &host, sums) == RTW_OK);
    CHECK(check(h, rays, n, nullptr, &dev, sums) == RTW_OK);
    CHECK(check(h, rays, n, rng, &host1, sums) == RTW_OK);
    CHECK(check(h, rays, n, rng, &dev1, sums) == RTW_OK);
    // null pointers
    CHECK(check(nullptr, rays, n, nullptr, &host, sums) == RTW_ERR_INVALID);
    CHECK(std::strstr(rtw_last_error(), "rtw_trace_radiance") != nullptr);
    CHECK(check(h, rays, n, nullptr, nullptr, sums) == RTW_ERR_INVALID);
    CHECK(check(h, nullptr, n, nullptr, &host, sums) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, nullptr, &host, nullptr) == RTW_ERR_INVALID);
    // n == 0: a no-op whatever the buffers, after the handle, params, build, precision and ranges
    CHECK(check(h, nullptr, 0, nullptr, &host, nullptr) == RTW_OK);
    CHECK(check(nullptr, nullptr, 0, nullptr, &host, nullptr) == RTW_ERR_INVALID);
    // precision, the strict build
    rtw_radiance_params fp32 = host;
    fp32.precision = RTW_PRECISION_FP32;
    CHECK(check(h, rays, n, nullptr, &fp32, sums) == RTW_ERR_UNSUPPORTED);
    CHECK(check(h, nullptr, 0, nullptr, &fp32, nullptr) == RTW_ERR_UNSUPPORTED);
    fp32.precision = 7;
    CHECK(check(h, rays, n, nullptr, &fp32, sums) == RTW_ERR_UNSUPPORTED);
    CHECK(check(h, rays, n, nullptr, &host, sums, true) == RTW_ERR_UNSUPPORTED);
    // the sample range and the depth
    {
        rtw_radiance_params p = host;
        p.spp_count = 0;
        CHECK(check(h, rays, n, nullptr, &p, sums) == RTW_ERR_INVALID);
        p.spp_count = -1;
        CHECK(check(h, rays, n, nullptr, &p, sums) == RTW_ERR_INVALID);
        p = host, p.spp_begin = -1;
        CHECK(check(h, rays, n, nullptr, &p, sums) == RTW_ERR_INVALID);
        p = host, p.max_depth = -1;
        CHECK(check(h, rays, n, nullptr, &p, sums) == RTW_ERR_INVALID);
        p = host, p.max_depth = 0;
        CHECK(check(h, rays, n, nullptr, &p, sums) == RTW_OK);
        p = host, p.spp_begin = 0x7fffffff - 2, p.spp_count = 2;
        CHECK(check(h, rays, n, nullptr, &p, sums) == RTW_OK);
        p.spp_count = 3;
        CHECK(check(h, rays, n, nullptr, &p, sums) == RTW_ERR_INVALID);
    }
    // caller-supplied states start one sample per ray
    CHECK(check(h, rays, n, rng, &host, sums) == RTW_ERR_INVALID);
    CHECK(std::strstr(rtw_last_error(), "spp_count") != nullptr);
    // keys and counts (the buffers are not touched by the checks: no overlap at these sizes is claimed, so
    // the ray buffer is placed far from the sums)
    {
        const char* far_rays = reinterpret_cast<const char*>(uintptr_t(1) << 44);
        const char* far_sums = reinterpret_cast<const char*>(uintptr_t(1) << 46);
        rtw_radiance_params p = params(50, 0, 1, false, 0);
        CHECK(check(h, far_rays, 0xffffffffull, nullptr, &p, far_sums) == RTW_OK);
        CHECK(check(h, far_rays, 1ull << 32, nullptr, &p, far_sums) == RTW_ERR_INVALID);
        p.first_key = 1;
        CHECK(check(h, far_rays, 0xffffffffull, nullptr, &p, far_sums) == RTW_OK);  // keys 1 .. 2^32 - 1
        p.first_key = 2;
        CHECK(check(h, far_rays, 0xffffffffull, nullptr, &p, far_sums) == RTW_ERR_INVALID);
        p.first_key = 0xffffffffu;
        CHECK(check(h, rays, 1, nullptr, &p, sums) == RTW_OK);
        CHECK(check(h, rays, 2, nullptr, &p, sums) == RTW_ERR_INVALID);
        CHECK(std::strstr(rtw_last_error(), "first_key") != nullptr);
        CHECK(check(h, nullptr, 0, nullptr, &p, nullptr) == RTW_OK);
    }
    // misaligned device pointers (host pointers need no alignment)
    CHECK(check(h, buf + 8, n, nullptr, &dev, sums) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, nullptr, &dev, buf + 1024 + 4) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, nullptr, &dev, buf + 1024 + 8) == RTW_OK);
    CHECK(check(h, rays, n, buf + 2050, &dev1, sums) == RTW_ERR_INVALID);
    CHECK(check(h, buf + 8, n, buf + 2050, &host1, buf + 1024 + 4) == RTW_OK);
    // overlaps: the sums over the rays or the states (one shared byte is enough)
    CHECK(check(h, rays, n, nullptr, &host, rays) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, nullptr, &host, buf + 511) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, nullptr, &host, buf + 512) == RTW_OK);
    CHECK(check(h, buf + 64, n, nullptr, &host, buf) == RTW_ERR_INVALID);  // the sums end inside the rays
    CHECK(check(h, rays, n, buf + 1024 + 188, &host1, sums) == RTW_ERR_INVALID);
    CHECK(std::strstr(rtw_last_error(), "overlap") != nullptr);
    CHECK(check(h, rays, n, buf + 1024 + 192, &host1, sums) == RTW_OK);

    // ---- rtw_radiance_plan ---------------------------------------------------------------
    const size_t big = ~size_t(0) >> 1;  // no budget: the 32-bit pass-local id alone cuts
    const uint64_t M = 0xffffffffull;
    plan_case(0, dev, false, size_t(1) << 30, kRadianceStageBytes, kRadianceChunkMax);
    plan_case(8, params(0, 0, 4, true), false, size_t(1) << 30, kRadianceStageBytes, kRadianceChunkMax);
    for (int staged = 0; staged < 2; ++staged) {
        plan_case(1, params(50, 2, 3, !staged), false, size_t(1) << 30, kRadianceStageBytes, kRadianceChunkMax);
        plan_case(1, params(50, 0, 1, !staged), true, size_t(1) << 30, kRadianceStageBytes, kRadianceChunkMax);
        plan_case(1000, params(50, 2, 3, !staged), false, size_t(1) << 30, kRadianceStageBytes, kRadianceChunkMax);
        // n * spp = 2^32 - 1 (= 3 * 1431655765) and 2^32 (= 4 * 2^30): one pass, then two
        plan_case(1431655765ull, params(50, 0, 3, !staged), false, big, big, kRadianceChunkMax);
        plan_case(1ull << 30, params(50, 0, 4, !staged), false, big, big, kRadianceChunkMax);
        // the most rays of a call: more than a chunk holds
        plan_case(M, params(50, 0, 1, !staged, 0), true, big, big, kRadianceChunkMax);
        plan_case(M, params(50, 5, 2, !staged, 1), false, size_t(1) << 30, kRadianceStageBytes, kRadianceChunkMax);
        // small bounds: many chunks, several passes per chunk, uneven tails
        plan_case(1000, params(50, 1, 7, !staged, 4000000000u), false, 2500, 92 * 300, 333);
        plan_case(1000, params(50, 0, 1, !staged), true, 7, 1, 1000);
        plan_case(65, params(3, 0, 5, !staged), false, 64, kRadianceStageBytes, 64);
    }
    {
        const radiance_plan A = rtw_radiance_plan(1431655765ull, params(50, 0, 3, true), false, big);
        radiance_chunk ch;
        CHECK(A.n_chunks == 1 && rtw_radiance_chunk(A, 0, &ch) == RTW_OK && ch.call.pass_spp == 3);
        const radiance_plan B = rtw_radiance_plan(1ull << 30, params(50, 0, 4, true), false, big);
        CHECK(B.n_chunks == 1 && rtw_radiance_chunk(B, 0, &ch) == RTW_OK && ch.call.pass_spp == 3);  // 3 + 1 samples
        const radiance_plan D = rtw_radiance_plan(M, params(50, 0, 1, true), false, big);
        CHECK(D.n_chunks == 3 && D.chunk_rays == kRadianceChunkMax);
        // the defaults: what the entry point stages
        const radiance_plan H = rtw_radiance_plan(2000000, params(50, 0, 1, false), true, size_t(1) << 30);
        CHECK(H.chunk_rays == kRadianceStageBytes / 92 && H.n_chunks == 3);
    }

    // ---- select_rays -------------------------------------------------------------------------
    const int masks[] = {0, SF_CHECKER, SF_METAL, SF_DIEL, SF_METAL | SF_DIEL, SF_NOISE, SF_NOCHECKER, SF_ALL,
                         SF_IMAGE | SF_DIEL};
    const uint32_t bytes[] = {1024, 41 * 1024};
    const int stack_nodes[3][2] = {{kLdsStack, 1000}, {kLdsStack + 1, 1000}, {kLdsStack, 65536}};
    for (int strict = 0; strict < 2; ++strict)
        for (int sort = -1; sort < 2; ++sort)
            for (int f = 0; f < 8; ++f)
                for (int mask : masks)
                    for (uint32_t b : bytes)
                        for (auto& sn : stack_nodes)
                            for (int bits = 0; bits < 32; ++bits)
                                for (int wavefront = 0; wavefront < 2; ++wavefront)
                                    for (int split = 0; split < 2; ++split) {
                                        select_in s;
                                        s.features = f, s.shade_mask = mask, s.shade_bytes = b;
                                        s.stack_need = sn[0], s.n_nodes = sn[1];
                                        s.ysph = bits & 1, s.static_scene = bits & 2, s.lights = bits & 4;
                                        s.black = bits & 8, s.pin = bits & 16;
                                        s.env.wavefront = wavefront, s.env.split = split, s.env.sort = sort;
                                        s.strict = strict;
                                        check_rays(s);
                                    }
    // every row carries the bit, no F_PIN, and is some whole-image row with the bit
    CHECK(kPersistRaysList.size() == 4);
    for (const active_inst& a : kPersistRaysList)
        CHECK((a.id.f & F_RAYS) && !(a.id.f & (F_PIN | F_ACTIVE)) &&
              index_of(kPersistList, inst{a.id.f & ~F_RAYS, a.id.m, a.id.l}) >= 0);
    // the built-in scenes' facts (as select_active_check.cpp has them) get their rows by default
    struct {
        const char* name;
        select_in s;
        const char* want;
    } scenes[4];
    scenes[0].name = "cornell_box", scenes[0].want = "k_persist_sort<1136, 8, true>";
    scenes[0].s.shade_mask = SF_DIEL, scenes[0].s.shade_bytes = scenes[0].s.f32_bytes = 4608;
    scenes[0].s.static_scene = scenes[0].s.lights = scenes[0].s.black = true;
    scenes[1].name = "random_balls", scenes[1].want = "k_persist_sort<1160, 12, false>";
    scenes[1].s.shade_mask = SF_METAL | SF_DIEL, scenes[1].s.shade_bytes = scenes[1].s.f32_bytes = 64 * 1024;
    scenes[1].s.ysph = true;
    scenes[2].name = "random_balls/bvh", scenes[2].want = "k_persist<1154, 12, false, true>";
    scenes[2].s = scenes[1].s;
    scenes[2].s.features = F_WBVH, scenes[2].s.stack_need = 12, scenes[2].s.n_nodes = 969;
    scenes[3].name = "book2_final/bvh", scenes[3].want = "k_persist<1125, 29, false, true>";
    scenes[3].s.features = F_MEDIA | F_GBVH, scenes[3].s.shade_mask = SF_NOCHECKER;
    scenes[3].s.shade_bytes = scenes[3].s.f32_bytes = 64 * 1024;
    scenes[3].s.stack_need = 12, scenes[3].s.group_depth = 12, scenes[3].s.n_nodes = 1668;
    scenes[3].s.lights = scenes[3].s.black = scenes[3].s.pin = true;
    for (auto& x : scenes) {
        const kernel_choice c = select_rays(x.s);
        std::printf("scene %s: %s\n", x.name, c.name.c_str());
        CHECK(c.name == x.want && c.persistent());
        select_in w = x.s;
        w.env.wavefront = true;
        CHECK(select_rays(w).name.rfind("k_regen_rays + ", 0) == 0);
    }
    for (auto& k : g_kinds) std::printf("%s: %ld\n", k.first.c_str(), k.second);
    CHECK(g_kinds["persistent row"] > 0 && g_kinds["k_regen_rays + k_segment"] > 0 &&
          g_kinds["k_regen_rays + split pair"] > 0);
    if (fails) return 1;
    std::printf("OK (radiance_check)\n");
    return 0;
}
