// query.cpp — rtw_query_check_args and rtw_query_plan (query.h): plain C++, no HIP.
#include "query.h"
#include <algorithm>
#include <string>
#include "rtw_host_util.h"

namespace {
bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }
}  // namespace

int rtw_query_check_args(const char* what, const void* handle, const void* rays, uint64_t n, const void* rng,
                         const rtw_query_params* params, const void* out, size_t out_stride, bool has_media,
                         bool strict_build) {
    const std::string w = what;
    if (!handle) return rtw_fail(RTW_ERR_INVALID, w + ": null scene handle");
    if (!params) return rtw_fail(RTW_ERR_INVALID, w + ": null params");
    if (strict_build) return rtw_fail(RTW_ERR_UNSUPPORTED, w + ": the strict-radiance build has no query kernels");
    if (params->precision != RTW_PRECISION_FP64)
        return rtw_fail(RTW_ERR_UNSUPPORTED, w + ": ray queries are fp64 only (precision must be RTW_PRECISION_FP64)");
    if (n == 0) return RTW_OK;
    if (!rays || !out) return rtw_fail(RTW_ERR_INVALID, w + ": null ray or output buffer");
    if (has_media && !rng)
        return rtw_fail(RTW_ERR_INVALID, w + ": the scene has media, whose free-flight draws need the rng states");
    const void* const r = has_media ? rng : nullptr;
    if (params->on_device) {
        if (misaligned(rays, 16) || (out_stride == sizeof(rtw_query_hit) && misaligned(out, 16)))
            return rtw_fail(RTW_ERR_INVALID, w + ": device ray and hit buffers must be 16-byte aligned");
        if (r && misaligned(r, 4)) return rtw_fail(RTW_ERR_INVALID, w + ": the device rng buffer must be 4-byte aligned");
    }
    // (byte counts must not overflow; no buffer holds 2^57 rays)
    if (n >= (1ull << 57)) return rtw_fail(RTW_ERR_INVALID, w + ": too many rays");
    const size_t nr = (size_t)n * sizeof(rtw_query_ray), no = (size_t)n * out_stride, ng = (size_t)n * 4;
    if (rtw_spans_overlap(rays, nr, out, no) || (r && (rtw_spans_overlap(r, ng, out, no) || rtw_spans_overlap(r, ng, rays, nr))))
        return rtw_fail(RTW_ERR_INVALID, w + ": two of the ray, output and rng buffers overlap");
    return RTW_OK;
}

int rtw_query_check_camera_args(const void* rays, const void* rng_out, uint64_t capacity, uint64_t total,
                                bool on_device) {
    if (!rays) return rtw_fail(RTW_ERR_INVALID, "rtw_camera_rays: null ray buffer");
    if (total > 0xffffffffull) return rtw_fail(RTW_ERR_INVALID, "rtw_camera_rays: more than 2^32 - 1 rays in one call");
    if (capacity < total)
        return rtw_fail(RTW_ERR_INVALID, "rtw_camera_rays: capacity " + std::to_string(capacity) + " below the " +
                                             std::to_string(total) + " rays of the call");
    if (on_device && (misaligned(rays, 16) || (rng_out && misaligned(rng_out, 4))))
        return rtw_fail(RTW_ERR_INVALID, "rtw_camera_rays: device buffers must be 16-byte (rays) and 4-byte (rng) aligned");
    if (rng_out && total && rtw_spans_overlap(rays, (size_t)total * sizeof(rtw_query_ray), rng_out, (size_t)total * 4))
        return rtw_fail(RTW_ERR_INVALID, "rtw_camera_rays: rays and rng_out overlap");
    return RTW_OK;
}

query_plan rtw_query_plan(uint64_t n, bool staged, size_t out_stride, bool with_rng, size_t stage_bytes,
                          uint64_t launch_max) {
    query_plan P;
    P.n = n;
    P.staged = staged;
    if (n == 0) return P;
    launch_max = std::max<uint64_t>(1, std::min<uint64_t>(launch_max, kQueryLaunchMax));
    P.chunk_rays = n;
    if (staged) {
        const size_t ray_bytes = sizeof(rtw_query_ray) + out_stride + (with_rng ? 4 : 0);
        P.chunk_rays = std::min<uint64_t>(n, std::max<uint64_t>(1, stage_bytes / ray_bytes));
        P.bytes_rays = (size_t)P.chunk_rays * sizeof(rtw_query_ray);
        P.bytes_out = (size_t)P.chunk_rays * out_stride;
        P.bytes_rng = with_rng ? (size_t)P.chunk_rays * 4 : 0;
    }
    P.n_chunks = (n + P.chunk_rays - 1) / P.chunk_rays;
    P.launch_rays = std::min<uint64_t>(P.chunk_rays, launch_max);
    return P;
}

query_span rtw_query_chunk(const query_plan& P, uint64_t c) {
    query_span s;
    s.first = c * P.chunk_rays;
    s.count = std::min<uint64_t>(P.chunk_rays, P.n - s.first);
    return s;
}

uint64_t rtw_query_launches(const query_plan& P, const query_span& chunk) {
    return chunk.count ? (chunk.count + P.launch_rays - 1) / P.launch_rays : 0;
}

query_span rtw_query_launch(const query_plan& P, const query_span& chunk, uint64_t l) {
    query_span s;
    s.first = chunk.first + l * P.launch_rays;
    s.count = std::min<uint64_t>(P.launch_rays, chunk.first + chunk.count - s.first);
    return s;
}
