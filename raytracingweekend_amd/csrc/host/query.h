// query.h — the host side of rtw_query.h that needs no device: the refusals of
// a ray query's arguments and how its n rays are cut into kernel launches and,
// for host buffers, into staged chunks.  Pure functions (no HIP, no
// environment): the entry points in rtw_kernels.hip call them, and
// tests/cpp/query_check.cpp checks them on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include "rtw_query.h"

// Most rays of one launch.  The kernels index a launch's rays with 32 bits and
// step by the grid's threads: below 2^31 + a grid's threads nothing wraps.
constexpr uint64_t kQueryLaunchMax = 1ull << 31;
// Bytes of the handle's staging buffers a host-buffer query may hold at once
// (rays, outputs and rng states of one chunk together).
constexpr size_t kQueryStageBytes = size_t(64) << 20;

// Every refusal of rtw_trace_closest / rtw_trace_occluded that needs no
// device, in this order: a null handle or params (RTW_ERR_INVALID); the strict
// build, a precision other than FP64 (RTW_ERR_UNSUPPORTED); then n == 0 is
// RTW_OK whatever the buffers; null rays or out, media without rng, on_device
// with rays / out (out_stride 64: hits) not 16-byte or rng not 4-byte aligned,
// two of rays, out and rng overlapping (RTW_ERR_INVALID).  out_stride: bytes
// per ray of the output (64 hits, 1 occlusion flags).  rng is checked only
// when the scene has media (else it is never touched).
int rtw_query_check_args(const char* what, const void* handle, const void* rays, uint64_t n, const void* rng,
                         const rtw_query_params* params, const void* out, size_t out_stride, bool has_media,
                         bool strict_build);

// ... of rtw_camera_rays beyond rtw_plan_call's: null rays, fewer than
// `total` = spp_count * npix rays of capacity, more than 2^32 - 1 rays,
// on_device alignment, rays and rng_out overlapping.
int rtw_query_check_camera_args(const void* rays, const void* rng_out, uint64_t capacity, uint64_t total,
                                bool on_device);

struct query_span {
    uint64_t first = 0, count = 0;  // rays [first, first + count)
};

// n rays as chunks, each chunk as launches.  Device buffers: one chunk, [0, n).
// Host buffers (staged): chunks of at most stage_bytes / ray_bytes rays (one at
// least), copied through the handle's buffers of bytes_* bytes; ray_bytes = 64
// + out_stride + (with_rng ? 4 : 0).  No launch holds more than launch_max
// rays, and the launches of the chunks tile [0, n) exactly once, in order.
struct query_plan {
    uint64_t n = 0;
    bool staged = false;
    uint64_t chunk_rays = 0;  // rays of every chunk but the last
    uint64_t n_chunks = 0;    // 0 for n == 0
    uint64_t launch_rays = 0; // rays of every launch of a chunk but its last
    size_t bytes_rays = 0, bytes_out = 0, bytes_rng = 0;  // staging buffers (0: not staged / no rng)
};
query_plan rtw_query_plan(uint64_t n, bool staged, size_t out_stride, bool with_rng,
                          size_t stage_bytes = kQueryStageBytes, uint64_t launch_max = kQueryLaunchMax);
query_span rtw_query_chunk(const query_plan& P, uint64_t c);                 // chunk c of [0, n_chunks)
uint64_t rtw_query_launches(const query_plan& P, const query_span& chunk);    // launches of a chunk
query_span rtw_query_launch(const query_plan& P, const query_span& chunk, uint64_t l);
