/*
 * rtw_query.h — ray queries for the MI355X path tracer: trace rays the CALLER
 * supplies against an uploaded scene, closest hit or occlusion, and obtain the
 * camera rays a render would trace.  For picking, depth and visibility maps,
 * shadow tests and collision probes, and for checking device traversal ray by
 * ray.  An addition to rtw_denoise.h (same library, same conventions, same
 * RTW_ABI_VERSION: new symbols only, no struct of the other headers changes).
 *
 * All arithmetic is the renders' IEEE double traversal (fp64 only, see
 * rtw_query_params.precision): the walk is the device function the render
 * kernels call, started at the ray's t_max instead of DBL_MAX.
 *
 * ---- records -----------------------------------------------------------------
 * Both records are 64 bytes.  Device buffers must be 16-byte aligned (the
 * kernels move a record as four 16-byte loads / stores per lane).
 *
 * ---- rtw_trace_closest, operation by operation ---------------------------------
 * For ray k = rays[k], r = ray(o, d, time):
 *   1. if !(t_max > 0.001f) (too small, negative or NaN): a miss, no walk.
 *   2. else the result of world->hit(r, 0.001f, t_max, rec) of the scene graph
 *      the handle was flattened from (hittable_list::hit with both its walks,
 *      bvh_node::hit for a BVH: the same winner, ties by list order).  t_min is
 *      the reference's float literal.  Equality at t_max is the reference's: a
 *      rect at exactly t_max is accepted (t > t1 rejects), a sphere is not
 *      (temp < t_max accepts).  t_max = +inf is allowed.
 *   3. on a hit: t, p, n = rec.t, rec.p, rec.normal after the enclosing
 *      transforms (as Normal mode shows n); material = the material index;
 *      prim = the winning prim index.  A constant_medium's hit: prim =
 *      -(2 + entry), material = that entry's phase_material, n = (1,0,0)
 *      through the enclosing ops.
 *   4. on a miss: prim = material = -1, t = t_max as given, p = n = 0.
 *
 * rng[k] is the std::minstd_rand state ray k draws from (the state
 * rtw_path_seed starts).  Only a scene with media draws (the free-flight
 * distances of both world walks): then rng is read and written back, and NULL
 * is RTW_ERR_INVALID.  A scene without media never touches it; it may be NULL.
 *
 * ---- rtw_trace_occluded -------------------------------------------------------
 * occluded[k] = 1 exactly when rtw_trace_closest reports a hit for ray k, else
 * 0.  With media the closest walk runs unchanged, so the draws and the rng
 * states left behind are rtw_trace_closest's.
 *
 * ---- moving spheres under a BVH ---------------------------------------------
 * The BVH boxes of moving spheres cover the desc camera's shutter only, so in
 * a scene with a BVH and moving spheres a ray whose time lies outside
 * [min(time0, time1), max(time0, time1)] of the desc camera (or is NaN) cannot
 * be traced: the kernel counts such rays, the call returns RTW_ERR_INVALID
 * after its synchronise and the outputs are then unspecified (host and device
 * buffers alike).
 */
#ifndef RTW_QUERY_H
#define RTW_QUERY_H

#include "rtw_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtw_query_ray {
    double o[3];  /* origin                                                  */
    double d[3];  /* direction (any length: t is in its units)               */
    double time;  /* ray time (moving spheres)                               */
    double t_max; /* the hit's t lies in (0.001f, t_max]; +inf allowed      */
} rtw_query_ray; /* 64 bytes */

typedef struct rtw_query_hit {
    double t;         /* hit: rec.t; miss: the ray's t_max as given          */
    double p[3];      /* hit point; 0 on a miss                              */
    double n[3];      /* the hit record's normal; 0 on a miss                */
    int32_t prim;     /* prim index; -(2 + entry) for a medium; -1 miss      */
    int32_t material; /* material index; -1 on a miss                        */
} rtw_query_hit; /* 64 bytes */

typedef struct rtw_query_params {
    int32_t on_device; /* 1: all buffers are device memory of the handle's GPU */
    int32_t precision; /* RTW_PRECISION_FP64 only (an fp32 query has no agreed
                          tolerance yet: RTW_ERR_UNSUPPORTED)                */
    int32_t pad[2];
} rtw_query_params; /* 16 bytes */

/* Closest hit of n rays (above).  Host buffers are staged through the handle
 * in chunks of bounded size; device buffers are read and written in place.
 * Stream-ordered after the handle's renders; returns when hits is written.
 * out_stats: samples = segments = n, ms_total from events (staging copies
 * included for host buffers), launches_intersect.
 * RTW_ERR_INVALID: a null handle, rays, params or hits (n > 0); rng NULL for a
 * scene with media; on_device with a pointer that is not 16-byte aligned (rng:
 * 4) or not memory of the handle's GPU; an output overlapping an input or the
 * other output; a ray time outside the shutter (above).  n == 0 is a
 * successful no-op.  RTW_ERR_UNSUPPORTED: precision other than FP64; the
 * strict-radiance build (as rtw_render_features). */
int rtw_trace_closest(void* scene_handle, const rtw_query_ray* rays, uint64_t n, uint32_t* rng /* may be NULL */,
                      const rtw_query_params* params, rtw_query_hit* hits, rtw_stats* out_stats /* may be NULL */);

/* occluded[k] = 1 iff rtw_trace_closest reports a hit for ray k (one byte per
 * ray).  Arguments, refusals and stats as rtw_trace_closest. */
int rtw_trace_occluded(void* scene_handle, const rtw_query_ray* rays, uint64_t n, uint32_t* rng /* may be NULL */,
                       const rtw_query_params* params, uint8_t* occluded, rtw_stats* out_stats /* may be NULL */);

/* The rays rtw_render_accumulate traces first for the samples and rows params
 * selects: the same rtw_path_seed stream, jitter, lens and time draws.  Sample
 * s of the pixel (i, row) of the call's row-th selected row (j = row_begin +
 * row * row_step) is written at
 *     q = (s - spp_begin) * npix + row * nx + i,   npix = selected rows * nx,
 * the render's pass-local sample id, with t_max = +inf; rng_out[q] (may be
 * NULL) is the stream's state after the camera's draws, the state
 * rtw_trace_closest continues from.  params->accum_on_device says where rays
 * and rng_out live (device: 16- and 4-byte aligned); precision and max_depth
 * are not read.  RTW_ERR_INVALID: what rtw_render_accumulate refuses, capacity
 * below spp_count * npix, more than 2^32 - 1 rays.  RTW_ERR_UNSUPPORTED in the
 * strict-radiance build. */
int rtw_camera_rays(void* scene_handle, const rtw_camera_desc* camera, const rtw_render_params* params,
                    rtw_query_ray* rays, uint32_t* rng_out /* may be NULL */, uint64_t capacity);

/* The kernels that rtw_trace_closest ("k_query<F>") and rtw_trace_occluded
 * ("k_occluded<F>"; with media it runs k_query's walk and stores the flag)
 * launch for this handle, named as rtw_scene_query_features names kernels. */
int rtw_scene_query_trace(void* scene_handle, char closest[128], char occluded[128]);

#ifdef __cplusplus
}
#endif

#endif /* RTW_QUERY_H */
