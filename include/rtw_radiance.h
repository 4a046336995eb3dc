/*
 * rtw_radiance.h — radiance queries for the MI355X path tracer: path-trace rays
 * the CALLER supplies against an uploaded scene and obtain, per ray, the sum of
 * its samples' radiance.  For cameras the library does not have (fisheye,
 * panoramic, orthographic, stereo, a lens model of one's own), light probes and
 * irradiance samples, lightmap texels, and re-renders of paths picked out of an
 * image.  An addition to rtw_query.h (same library, same conventions, same
 * RTW_ABI_VERSION: new symbols only, no struct of the other headers changes).
 *
 * All arithmetic is the fp64 renders' (rtw_radiance_params.precision): a path
 * runs through the same traversal, materials, pdfs, media and RNG order as a
 * path of rtw_render_accumulate; only where it starts differs.
 *
 * ---- rtw_trace_radiance, operation by operation -------------------------------
 * For ray k = rays[k], r = ray(o, d, time), and sample s of
 * [spp_begin, spp_begin + spp_count):
 *   1. the stream of the sample is rtw_path_seed(seed, first_key + k, s), the
 *      std::minstd_rand state a render gives sample s of the pixel whose index
 *      is first_key + k.  Nothing draws from it first: there are no camera
 *      draws (no jitter, lens or time draw).
 *   2. the sample's value is color(r, world, lights, max_depth) of
 *      RayTracingWeekend.cpp:45-160 drawn from that stream, for the scene graph
 *      the handle was flattened from.  The record's t_max is NOT read: color()
 *      walks from DBL_MAX, so the output of rtw_camera_rays (t_max = +inf) and
 *      records made for rtw_trace_closest can be passed as they are.  The
 *      scene's render type (colour or normals) and its background follow from
 *      color() itself.
 *   3. v_k = ((0 + value(s0)) + value(s0 + 1)) + ... in increasing s, then
 *      sum_rgb[3k + c] += v_k[c]: the ADD semantics of rtw_render_accumulate
 *      (a second identical call doubles a sum that was zero).  A call that
 *      needs several passes adds the passes' samples in the same order.
 *
 * Caller-supplied streams (rng != NULL): ray k's single sample starts from the
 * state rng[k], taken as given (as rtw_trace_closest takes it); spp_count must
 * then be 1 and spp_begin, seed and first_key are not read.  rng is not written.
 * rtw_camera_rays leaves exactly these states, so
 *     rtw_camera_rays(..., rays, rng_out, ...);
 *     rtw_trace_radiance(h, rays, n, rng_out, {spp_count = 1, ...}, sums, ...)
 * traces the render's own paths: per-pixel sums of these sums in sample order
 * are rtw_render_accumulate's, bit for bit.
 *
 * max_depth == 0: color() returns 0 at once, every sum is unchanged, nothing is
 * launched (the samples still count in out_stats).
 *
 * ---- moving spheres under a BVH ---------------------------------------------
 * As rtw_query.h: in a scene with a BVH and moving spheres a ray whose time lies
 * outside the desc camera's shutter (or is NaN) cannot be traced.  Such rays are
 * counted on the device, chunk by chunk, before the chunk is traced; the call
 * then returns RTW_ERR_INVALID and sum_rgb is unspecified (a call of one chunk,
 * which is every call below 2^30 rays in device buffers, leaves it unchanged).
 */
#ifndef RTW_RADIANCE_H
#define RTW_RADIANCE_H

#include "rtw_query.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtw_radiance_params {
    int32_t  max_depth;        /* color()'s depth argument; 0: every sum is 0, no launch        */
    int32_t  spp_begin;        /* samples [spp_begin, spp_begin + spp_count) of every ray        */
    int32_t  spp_count;        /* >= 1                                                           */
    int32_t  on_device;        /* 1: rays, rng and sum_rgb are device memory of the handle's GPU */
    uint64_t seed;
    uint32_t first_key;        /* ray k's RNG key is first_key + k (must not wrap)               */
    int32_t  precision;        /* RTW_PRECISION_FP64 only; FP32: RTW_ERR_UNSUPPORTED             */
    int32_t  wavefront_paths;  /* paths in flight, as in rtw_render_params: 0 = default          */
    int32_t  pad;
} rtw_radiance_params; /* 40 bytes */

/* Per-ray radiance sums of n rays (above).  Host buffers are staged through the
 * handle in chunks of bounded size; device buffers are read and written in
 * place.  Rays are traced in chunks whose passes hold at most 2^32 - 1 samples
 * and the per-pass radiance records rtw_render_accumulate allows itself; the
 * chunking changes no result (ray k's key is first_key + k wherever it falls).
 * Stream-ordered after the handle's renders; returns when sum_rgb is written.
 * out_stats: samples = n * spp_count, segments = world hit queries counted on
 * the device as for renders, launches_intersect, ms_total from events (staging
 * copies included).
 * RTW_ERR_INVALID: a null handle or params; with n > 0 null rays or sum_rgb;
 * spp_count < 1, spp_begin < 0, max_depth < 0, spp_begin + spp_count above
 * 2^31 - 1; first_key + n above 2^32; n above 2^32 - 1; rng with spp_count != 1;
 * on_device with a misaligned pointer (rays 16 bytes, sum_rgb 8, rng 4) or one
 * that is not memory of the handle's GPU; sum_rgb overlapping rays or rng; a
 * ray time outside the shutter (above).  n == 0 is a successful no-op.
 * RTW_ERR_UNSUPPORTED: precision other than FP64; the strict-radiance build. */
int rtw_trace_radiance(void* scene_handle, const rtw_query_ray* rays, uint64_t n,
                       const uint32_t* rng /* may be NULL */,
                       const rtw_radiance_params* params, double* sum_rgb,
                       rtw_stats* out_stats /* may be NULL */);

/* The kernel(s) an rtw_trace_radiance call on this handle launches under the
 * current environment (RTW_MODE, RTW_SORT, RTW_SPLIT as for renders): a
 * persistent kernel compiled for caller rays ("k_persist_sort<1136, 8, true>"),
 * or "k_regen_rays + " and the wavefront kernel it refills. */
int rtw_scene_query_radiance(void* scene_handle, char name[128]);

#ifdef __cplusplus
}
#endif

#endif /* RTW_RADIANCE_H */
