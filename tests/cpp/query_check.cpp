// query_check.cpp — csrc/host/query.cpp on the CPU: every refusal of
// rtw_query_check_args and rtw_query_check_camera_args, and rtw_query_plan's
// launches and staged chunks (they tile [0, n) exactly once, in order, no launch
// above the 32-bit limit, no chunk above the byte bound).  Prints the records'
// sizes and offsets for tests/test_query.py, then "OK (query_check)".
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "query.h"
#include "rtw_host_util.h"

namespace {
int fails = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            ++fails;                                                 \
        }                                                            \
    } while (0)

int check(const void* h, const void* rays, uint64_t n, const void* rng, const rtw_query_params* p, const void* out,
          size_t stride, bool media, bool strict = false) {
    return rtw_query_check_args("query_check", h, rays, n, rng, p, out, stride, media, strict);
}

void plan_case(uint64_t n, bool staged, size_t stride, bool with_rng, size_t stage_bytes, uint64_t launch_max) {
    const query_plan P = rtw_query_plan(n, staged, stride, with_rng, stage_bytes, launch_max);
    const size_t ray_bytes = 64 + stride + (with_rng ? 4 : 0);
    uint64_t next = 0, launches = 0;
    CHECK(P.n == n && P.staged == staged);
    if (n == 0) CHECK(P.n_chunks == 0);
    if (!staged) CHECK(P.n_chunks == (n ? 1u : 0u) && P.bytes_rays == 0 && P.bytes_out == 0 && P.bytes_rng == 0);
    for (uint64_t c = 0; c < P.n_chunks; ++c) {
        const query_span ch = rtw_query_chunk(P, c);
        CHECK(ch.first == next && ch.count >= 1 && ch.first + ch.count <= n);
        if (staged) {
            // the byte bound (a bound below one ray's bytes still moves one ray at a time)
            CHECK(ch.count * ray_bytes <= stage_bytes || ch.count == 1);
            CHECK(ch.count * 64 <= P.bytes_rays && ch.count * stride <= P.bytes_out);
            CHECK(with_rng ? ch.count * 4 <= P.bytes_rng : P.bytes_rng == 0);
            CHECK(P.bytes_rays + P.bytes_out + P.bytes_rng <= stage_bytes || P.chunk_rays == 1);
        }
        uint64_t at = ch.first;
        const uint64_t nl = rtw_query_launches(P, ch);
        CHECK(nl >= 1);
        for (uint64_t l = 0; l < nl; ++l) {
            const query_span ls = rtw_query_launch(P, ch, l);
            CHECK(ls.first == at && ls.count >= 1);
            CHECK(ls.count <= launch_max && ls.count <= kQueryLaunchMax && ls.count <= 0xffffffffull);
            at += ls.count;
            ++launches;
        }
        CHECK(at == ch.first + ch.count);
        next = at;
    }
    CHECK(next == n);
    std::printf("plan n=%llu staged=%d stride=%zu rng=%d: %llu chunks, %llu launches\n", (unsigned long long)n, (int)staged,
                stride, (int)with_rng, (unsigned long long)P.n_chunks, (unsigned long long)launches);
}
}  // namespace

int main() {
    std::printf("sizeof rtw_query_ray %zu o %zu d %zu time %zu t_max %zu\n", sizeof(rtw_query_ray),
                offsetof(rtw_query_ray, o), offsetof(rtw_query_ray, d), offsetof(rtw_query_ray, time),
                offsetof(rtw_query_ray, t_max));
    std::printf("sizeof rtw_query_hit %zu t %zu p %zu n %zu prim %zu material %zu\n", sizeof(rtw_query_hit),
                offsetof(rtw_query_hit, t), offsetof(rtw_query_hit, p), offsetof(rtw_query_hit, n),
                offsetof(rtw_query_hit, prim), offsetof(rtw_query_hit, material));
    std::printf("sizeof rtw_query_params %zu on_device %zu precision %zu pad %zu\n", sizeof(rtw_query_params),
                offsetof(rtw_query_params, on_device), offsetof(rtw_query_params, precision),
                offsetof(rtw_query_params, pad));

    // ---- rtw_query_check_args ------------------------------------------------------
    alignas(64) static char buf[4096];
    int handle = 0;
    const void* h = &handle;
    rtw_query_params host{}, dev{};
    dev.on_device = 1;
    const void* rays = buf;           // 8 rays: 512 bytes
    const void* hits = buf + 1024;    // 8 hits
    const void* rng = buf + 2048;     // 8 states
    const uint64_t n = 8;
    CHECK(check(h, rays, n, nullptr, &host, hits, 64, false) == RTW_OK);
    CHECK(check(h, rays, n, rng, &host, hits, 64, true) == RTW_OK);
    CHECK(check(h, rays, n, rng, &dev, hits, 64, true) == RTW_OK);
    CHECK(check(h, rays, n, nullptr, &dev, buf + 1025, 1, false) == RTW_OK);  // flags need no alignment
    // null pointers
    CHECK(check(nullptr, rays, n, nullptr, &host, hits, 64, false) == RTW_ERR_INVALID);
    CHECK(std::strstr(rtw_last_error(), "query_check") != nullptr);
    CHECK(check(h, rays, n, nullptr, nullptr, hits, 64, false) == RTW_ERR_INVALID);
    CHECK(check(h, nullptr, n, nullptr, &host, hits, 64, false) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, nullptr, &host, nullptr, 64, false) == RTW_ERR_INVALID);
    // media without rng; a media-free scene never reads it
    CHECK(check(h, rays, n, nullptr, &host, hits, 64, true) == RTW_ERR_INVALID);
    CHECK(std::strstr(rtw_last_error(), "media") != nullptr);
    CHECK(check(h, rays, n, nullptr, &host, hits, 64, false) == RTW_OK);
    // n == 0: a no-op whatever the buffers, after the handle, params, build and precision
    CHECK(check(h, nullptr, 0, nullptr, &host, nullptr, 64, true) == RTW_OK);
    CHECK(check(nullptr, nullptr, 0, nullptr, &host, nullptr, 64, true) == RTW_ERR_INVALID);
    // precision, the strict build
    rtw_query_params fp32{};
    fp32.precision = RTW_PRECISION_FP32;
    CHECK(check(h, rays, n, nullptr, &fp32, hits, 64, false) == RTW_ERR_UNSUPPORTED);
    CHECK(check(h, nullptr, 0, nullptr, &fp32, nullptr, 64, false) == RTW_ERR_UNSUPPORTED);
    fp32.precision = 7;
    CHECK(check(h, rays, n, nullptr, &fp32, hits, 64, false) == RTW_ERR_UNSUPPORTED);
    CHECK(check(h, rays, n, nullptr, &host, hits, 64, false, true) == RTW_ERR_UNSUPPORTED);
    // misaligned device pointers (host pointers need no alignment)
    CHECK(check(h, buf + 8, n, nullptr, &dev, hits, 64, false) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, nullptr, &dev, buf + 1024 + 8, 64, false) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, buf + 2050, &dev, hits, 64, true) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, buf + 2050, &dev, hits, 64, false) == RTW_OK);  // not read without media
    CHECK(check(h, buf + 8, n, buf + 2050, &host, buf + 1024 + 8, 64, true) == RTW_OK);
    // overlaps: output over input (one shared byte is enough), rng over either
    CHECK(check(h, rays, n, nullptr, &host, rays, 64, false) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, nullptr, &host, buf + 511, 1, false) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, nullptr, &host, buf + 512, 1, false) == RTW_OK);
    CHECK(check(h, buf + 64, n, nullptr, &host, buf, 64, false) == RTW_ERR_INVALID);  // hits end inside the rays
    CHECK(check(h, rays, n, buf + 508, &host, hits, 64, true) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, buf + 1024 + 508, &host, hits, 64, true) == RTW_ERR_INVALID);
    CHECK(check(h, rays, n, buf + 508, &host, hits, 64, false) == RTW_OK);
    CHECK(check(h, rays, 1ull << 60, nullptr, &host, hits, 64, false) == RTW_ERR_INVALID);

    // ---- rtw_query_check_camera_args -------------------------------------------------
    CHECK(rtw_query_check_camera_args(rays, rng, 8, 8, false) == RTW_OK);
    CHECK(rtw_query_check_camera_args(rays, nullptr, 9, 8, true) == RTW_OK);
    CHECK(rtw_query_check_camera_args(nullptr, rng, 8, 8, false) == RTW_ERR_INVALID);
    CHECK(rtw_query_check_camera_args(rays, rng, 7, 8, false) == RTW_ERR_INVALID);
    CHECK(rtw_query_check_camera_args(rays, rng, ~0ull, 1ull << 32, false) == RTW_ERR_INVALID);
    CHECK(rtw_query_check_camera_args(rays, rng, ~0ull, 0xffffffffull, false) == RTW_ERR_INVALID);  // (they overlap at that size)
    CHECK(rtw_query_check_camera_args(buf + 8, rng, 8, 8, true) == RTW_ERR_INVALID);
    CHECK(rtw_query_check_camera_args(rays, buf + 2050, 8, 8, true) == RTW_ERR_INVALID);
    CHECK(rtw_query_check_camera_args(rays, buf + 500, 8, 8, false) == RTW_ERR_INVALID);

    // ---- rtw_query_plan ----------------------------------------------------------------
    const uint64_t sizes[] = {0, 1, (1ull << 31) - 1, 1ull << 31, (1ull << 32) + 5};
    for (uint64_t m : sizes) {
        plan_case(m, false, 64, false, kQueryStageBytes, kQueryLaunchMax);
        plan_case(m, false, 1, true, kQueryStageBytes, kQueryLaunchMax);
        plan_case(m, true, 64, true, kQueryStageBytes, kQueryLaunchMax);
        plan_case(m, true, 1, false, kQueryStageBytes, kQueryLaunchMax);
        plan_case(m, true, 0, true, size_t(1) << 30, kQueryLaunchMax);
    }
    // the defaults: what the entry points launch
    {
        const query_plan P = rtw_query_plan((1ull << 32) + 5, false, 64, false);
        CHECK(P.n_chunks == 1 && P.launch_rays == (1ull << 31) && rtw_query_launches(P, rtw_query_chunk(P, 0)) == 3);
        const query_plan H = rtw_query_plan(1000000, true, 64, true);
        CHECK(H.chunk_rays == kQueryStageBytes / 132 && H.n_chunks == 2 && H.bytes_rays == H.chunk_rays * 64);
    }
    // small bounds: many chunks, several launches per chunk, uneven tails
    plan_case(1000, true, 64, true, 132 * 7, 3);
    plan_case(1000, true, 1, false, 65 * 64, 64);
    plan_case(1000, false, 64, false, 0, 7);
    plan_case(5, true, 64, false, 1, 1);  // a bound below one ray
    plan_case(4097, false, 1, false, 0, 4096);
    // a launch bound above the kernels' limit is cut to it
    {
        const query_plan P = rtw_query_plan(1ull << 33, false, 64, false, kQueryStageBytes, ~0ull);
        CHECK(P.launch_rays == kQueryLaunchMax);
    }
    if (fails) return 1;
    std::printf("OK (query_check)\n");
    return 0;
}
