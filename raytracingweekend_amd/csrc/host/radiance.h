// radiance.h — the host side of rtw_radiance.h that needs no device: the
// refusals of a radiance query's arguments and how its n rays are cut into
// chunks (each with its own first key), a chunk into passes and, for host
// buffers, into staged copies.  Pure functions (no HIP, no environment): the
// entry point in rtw_kernels.hip calls them, and tests/cpp/radiance_check.cpp
// checks them on the CPU.  A chunk is planned by rtw_plan_call itself, as a
// render of an image one row high whose pixels are the chunk's rays: the pool,
// the passes and every buffer's bytes are render_plan.h's arithmetic.
#pragma once
#include <cstddef>
#include <cstdint>
#include "render_plan.h"
#include "rtw_radiance.h"

// Most rays of one chunk: a chunk's rays are the pixels of its plan, whose
// count rtw_plan_call keeps below 2^31.
constexpr uint64_t kRadianceChunkMax = (1ull << 31) - 1;
// Bytes of the handle's staging buffers a host-buffer call may hold at once
// (rays, sums and rng states of one chunk together): query.h's bound.
constexpr size_t kRadianceStageBytes = size_t(64) << 20;

// Every refusal of rtw_trace_radiance that needs no device, in this order: a
// null handle or params (RTW_ERR_INVALID); the strict build, a precision other
// than FP64 (RTW_ERR_UNSUPPORTED); spp_count < 1, spp_begin < 0, max_depth < 0,
// spp_begin + spp_count above 2^31 - 1, rng with spp_count != 1, n above
// 2^32 - 1, first_key + n above 2^32 (RTW_ERR_INVALID); then n == 0 is RTW_OK
// whatever the buffers; null rays or sum_rgb, on_device with rays not 16-byte,
// sum_rgb not 8-byte or rng not 4-byte aligned, sum_rgb overlapping rays or
// rng (RTW_ERR_INVALID).
int rtw_radiance_check_args(const void* handle, const void* rays, uint64_t n, const void* rng,
                            const rtw_radiance_params* params, const void* sum_rgb, bool strict_build);

// n rays as chunks of at most min(chunk_max, budget) rays, and for host buffers
// (staged) of at most stage_bytes / (64 + 24 + (with_rng ? 4 : 0)) rays (one at
// least), copied through buffers of bytes_* bytes.  budget: the samples a pass
// may hold (RTW_PASS_SAMPLES, as rtw_plan_call's).  The chunks tile [0, n)
// exactly once, in order.
struct radiance_plan {
    uint64_t n = 0;
    bool staged = false;
    bool noop = false;        // n == 0 or max_depth == 0: nothing is traced, no sum changes
    uint64_t samples = 0;     // n * spp_count (stats.samples)
    uint64_t chunk_rays = 0;  // rays of every chunk but the last
    uint64_t n_chunks = 0;    // 0 for a no-op
    size_t bytes_rays = 0, bytes_sums = 0, bytes_rng = 0;  // staging buffers (0: not staged / no rng)
    size_t budget = 0;
    rtw_radiance_params prm{};
};
radiance_plan rtw_radiance_plan(uint64_t n, const rtw_radiance_params& params, bool with_rng, size_t budget,
                                size_t stage_bytes = kRadianceStageBytes, uint64_t chunk_max = kRadianceChunkMax);

// Chunk c of [0, n_chunks): rays [first, first + count), whose RNG keys start
// at first_key = params.first_key + first, and its passes as rtw_plan_call
// plans a render of count x 1 pixels (R: that render's parameters; pass p
// starts after p * call.pass_spp samples per ray: rtw_plan_pass(call, R, done)).
struct radiance_chunk {
    uint64_t first = 0, count = 0;
    uint32_t first_key = 0;
    rtw_render_params R{};
    call_plan call;
};
int rtw_radiance_chunk(const radiance_plan& P, uint64_t c, radiance_chunk* out);
