// radiance.cpp — rtw_radiance_check_args and rtw_radiance_plan (radiance.h): plain C++, no HIP.
#include "radiance.h"
#include <algorithm>
#include <string>
#include "rtw_host_util.h"

namespace {
bool misaligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a != 0; }
const char* const kWhat = "rtw_trace_radiance";
int invalid(const std::string& msg) { return rtw_fail(RTW_ERR_INVALID, std::string(kWhat) + ": " + msg); }
}  // namespace

int rtw_radiance_check_args(const void* handle, const void* rays, uint64_t n, const void* rng,
                            const rtw_radiance_params* params, const void* sum_rgb, bool strict_build) {
    if (!handle) return invalid("null scene handle");
    if (!params) return invalid("null params");
    if (strict_build)
        return rtw_fail(RTW_ERR_UNSUPPORTED, std::string(kWhat) + ": the strict-radiance build has no query kernels");
    const rtw_radiance_params& p = *params;
    if (p.precision != RTW_PRECISION_FP64)
        return rtw_fail(RTW_ERR_UNSUPPORTED,
                        std::string(kWhat) + ": radiance queries are fp64 only (precision must be RTW_PRECISION_FP64)");
    if (p.spp_count < 1 || p.spp_begin < 0 || p.max_depth < 0) return invalid("bad sample range or max_depth");
    if ((int64_t)p.spp_begin + p.spp_count > 0x7fffffffll) return invalid("spp_begin + spp_count above 2^31 - 1");
    if (rng && p.spp_count != 1) return invalid("caller-supplied rng states start one sample per ray (spp_count must be 1)");
    if (n > 0xffffffffull) return invalid("more than 2^32 - 1 rays in one call");
    if ((uint64_t)p.first_key + n > (1ull << 32)) return invalid("first_key + n wraps the 32-bit RNG key");
    if (n == 0) return RTW_OK;
    if (!rays || !sum_rgb) return invalid("null ray or sum buffer");
    if (p.on_device) {
        if (misaligned(rays, 16)) return invalid("the device ray buffer must be 16-byte aligned");
        if (misaligned(sum_rgb, 8)) return invalid("the device sum buffer must be 8-byte aligned");
        if (rng && misaligned(rng, 4)) return invalid("the device rng buffer must be 4-byte aligned");
    }
    const size_t nr = (size_t)n * sizeof(rtw_query_ray), ns = (size_t)n * 24, ng = (size_t)n * 4;
    if (rtw_spans_overlap(rays, nr, sum_rgb, ns) || (rng && rtw_spans_overlap(rng, ng, sum_rgb, ns)))
        return invalid("sum_rgb overlaps the ray or rng buffer");
    return RTW_OK;
}

radiance_plan rtw_radiance_plan(uint64_t n, const rtw_radiance_params& params, bool with_rng, size_t budget,
                                size_t stage_bytes, uint64_t chunk_max) {
    radiance_plan P;
    P.n = n;
    P.staged = !params.on_device;
    P.prm = params;
    P.budget = budget;
    P.samples = n * (uint64_t)params.spp_count;
    if (n == 0 || params.max_depth <= 0) {
        P.noop = true;
        return P;
    }
    chunk_max = std::max<uint64_t>(1, std::min<uint64_t>(chunk_max, kRadianceChunkMax));
    P.chunk_rays = std::min<uint64_t>({n, chunk_max, std::max<uint64_t>(1, budget)});
    if (P.staged) {
        const size_t ray_bytes = sizeof(rtw_query_ray) + 24 + (with_rng ? 4 : 0);
        P.chunk_rays = std::min<uint64_t>(P.chunk_rays, std::max<uint64_t>(1, stage_bytes / ray_bytes));
        P.bytes_rays = (size_t)P.chunk_rays * sizeof(rtw_query_ray);
        P.bytes_sums = (size_t)P.chunk_rays * 24;
        P.bytes_rng = with_rng ? (size_t)P.chunk_rays * 4 : 0;
    }
    P.n_chunks = (n + P.chunk_rays - 1) / P.chunk_rays;
    return P;
}

int rtw_radiance_chunk(const radiance_plan& P, uint64_t c, radiance_chunk* out) {
    radiance_chunk ch;
    ch.first = c * P.chunk_rays;
    ch.count = std::min<uint64_t>(P.chunk_rays, P.n - ch.first);
    ch.first_key = P.prm.first_key + (uint32_t)ch.first;
    // the chunk as a render: count x 1 pixels, the call's samples of each
    rtw_render_params& R = ch.R;
    R.nx = (int32_t)ch.count, R.ny = 1;
    R.spp = P.prm.spp_begin + P.prm.spp_count;
    R.spp_begin = P.prm.spp_begin, R.spp_count = P.prm.spp_count;
    R.max_depth = P.prm.max_depth;
    R.seed = P.prm.seed;
    R.row_begin = 0, R.row_step = 1;
    R.accum_on_device = 1;  // (no whole-image staging: the sums are staged per chunk, above)
    R.wavefront_paths = P.prm.wavefront_paths;
    R.precision = RTW_PRECISION_FP64;
    const rtw_camera_desc no_camera{};  // (a ray-sourced job reads none)
    const layout_facts no_facts{};
    if (int rc = rtw_plan_call(R, no_camera, no_facts, nullptr, nullptr, P.budget, 0, &ch.call)) return rc;
    *out = ch;
    return RTW_OK;
}
