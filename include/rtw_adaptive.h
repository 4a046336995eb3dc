/*
 * rtw_adaptive.h — adaptive per-pixel sampling on the MI355X path tracer:
 * render more samples of a LIST of pixels, choose that list from the noise
 * map, and the loop that does both until every pixel is quiet or has taken
 * max_spp samples.  An addition to rtw_noise.h (same library, same
 * conventions, same RTW_ABI_VERSION: new symbols only, no struct of rtw_gpu.h
 * or rtw_noise.h changes).
 *
 * The engine is keyed by (seed, pixel, sample) and the accumulators hold raw
 * moments, so samples [a, b) of some pixels are well defined:
 * rtw_render_accumulate_active adds to the listed pixels exactly the bits
 * rtw_render_accumulate_moments adds to them with the same params.
 *
 * A pixel's index is p = j*nx + i, as in the accumulators.  counts[nx*ny] is
 * the number of samples each pixel has taken (uint32_t).  A pixel is ACTIVE
 * under (floor, target_rel, max_count) iff
 *     counts[p] < max_count, its six moments are finite, and
 *     counts[p] < 2  or  rel_p > target_rel,
 * rel_p being rtw_noise.h's expression evaluated with n = counts[p] (the same
 * operations in the same order).  A non-finite pixel is never active.
 *
 * BIAS.  The loop stops a pixel on a variance estimated from the very samples
 * it averages.  A dark pixel lit through a rare path (a caustic, a small
 * light seen by few paths) whose first samples all miss that path shows a
 * variance near zero, stops early and stays too dark: stopping on the
 * samples' own variance biases dark, heavy-tailed pixels LOW.  That is why
 * min_spp exists -- every pixel takes min_spp samples before any is judged --
 * and why `floor` keeps black pixels from being judged on relative error
 * alone.  Raise min_spp for scenes with caustics; the mean of a uniform
 * render has no such bias.
 */
#ifndef RTW_ADAPTIVE_H
#define RTW_ADAPTIVE_H

#include "rtw_noise.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Render samples [spp_begin, spp_begin + spp_count) of params (spp_count 0:
 * the rest of [spp_begin, spp)) of the n_active pixels listed in `active`:
 * pixel indices, strictly ascending, each below nx*ny.  For those pixels only
 * it ADDS to accum_rgb and to accum_sq_rgb (may be NULL) bit for bit what
 * rtw_render_accumulate_moments adds with the same params, and adds the
 * number of samples to counts[p] (may be NULL); nothing else in the buffers
 * is touched.  params->accum_on_device covers all four buffers, the list
 * included (a device list with host buffers: RTW_ERR_INVALID).
 * out_stats->samples == n_active * spp_count.  n_active == 0 is a no-op.
 * RTW_ERR_INVALID, before any render launch: row_begin != 0 or row_step > 1
 * (the list replaces row sharding), a list that is not strictly ascending or
 * out of range (a host list is checked on the host, a device list by a small
 * kernel: a duplicate would make the scatter-add a race), overlapping
 * buffers.  RTW_ERR_UNSUPPORTED: precision fp32 of a scene with image
 * textures, and the strict-radiance build. */
int rtw_render_accumulate_active(void* scene_handle, const rtw_camera_desc* camera, const rtw_render_params* params,
                                 const uint32_t* active, uint64_t n_active, double* accum_rgb,
                                 double* accum_sq_rgb /* may be NULL */, uint32_t* counts /* may be NULL */,
                                 rtw_stats* out_stats /* may be NULL */);

/* The ascending list of the active pixels (definition above) of host buffers
 * and its length; active_out holds up to nx*ny entries.  RTW_ERR_INVALID: a
 * null buffer, nx or ny <= 0, floor <= 0 or NaN, target_rel negative or NaN. */
int rtw_adaptive_select(const double* accum_rgb, const double* accum_sq_rgb, const uint32_t* counts, int nx, int ny,
                        double floor, double target_rel, uint32_t max_count, uint32_t* active_out,
                        uint64_t* n_active_out);

/* The same on the GPU for device buffers of the handle's device; the length
 * goes to host memory.  No atomics: per-block counts, an exclusive scan of
 * them and an ordered scatter on a grid that depends on nx*ny only, so the
 * list is rtw_adaptive_select's, element for element. */
int rtw_adaptive_select_device(void* scene_handle, const double* accum_dev, const double* accum_sq_dev,
                               const uint32_t* counts_dev, int nx, int ny, double floor, double target_rel,
                               uint32_t max_count, uint32_t* active_dev, uint64_t* n_active_host);

/* rtw_noise_estimate with a per-pixel n = counts[p].  Pixels with
 * counts[p] < 2 are left out and counted in `nonfinite` (NaN in the map).
 * With all counts equal to n >= 2 the map and the summary are the bits of
 * rtw_noise_estimate(..., n, ...). */
int rtw_noise_estimate_counts(const double* accum_rgb, const double* accum_sq_rgb, const uint32_t* counts, int nx,
                              int ny, double floor, double* stderr_rgb /* may be NULL */,
                              rtw_noise_summary* out /* may be NULL */);

/* ... and rtw_noise_estimate_device with counts (the same map bit for bit,
 * the summary in the same fixed order as rtw_noise_estimate_device's). */
int rtw_noise_estimate_counts_device(void* scene_handle, const double* accum_dev, const double* accum_sq_dev,
                                     const uint32_t* counts_dev, int nx, int ny, double floor,
                                     double* stderr_dev /* may be NULL */, rtw_noise_summary* out_host /* may be NULL */);

/* canvas = min(sqrt(sum / counts[p]), 1): rtw_finalize_canvas bit for bit
 * when the counts are uniform (a pixel without samples: NaN). */
int rtw_finalize_canvas_counts(const double* accum_rgb, const uint32_t* counts, int nx, int ny, double* canvas);
int rtw_finalize_canvas_counts_device(void* scene_handle, const double* accum_dev, const uint32_t* counts_dev, int nx,
                                      int ny, double* canvas_dev);

typedef struct rtw_adaptive_params {
    double target_rel; /* a pixel stops once rel_p <= target_rel (>= 0)          */
    double floor;      /* rtw_noise.h's floor (> 0)                              */
    int32_t min_spp;   /* samples every pixel takes before any is judged (>= 2)  */
    int32_t max_spp;   /* samples a pixel takes at most (>= min_spp)             */
    int32_t batch;     /* samples per later round; 0: as many as are done so far */
    int32_t pad;
} rtw_adaptive_params; /* 32 bytes */

typedef struct rtw_adaptive_result {
    uint64_t samples;        /* camera samples rendered: the sum of counts        */
    uint64_t pixels_at_max;  /* pixels that took max_spp samples                  */
    uint32_t rounds;         /* render rounds, round 0 included                   */
    uint32_t pad;
    rtw_noise_summary final; /* rtw_noise_estimate_counts of the result           */
} rtw_adaptive_result; /* 64 bytes */

/* The loop's schedule, a pure function: the sample range [*begin, *begin +
 * *count) of the round that follows `done` samples per active pixel.  Round 0
 * (done == 0) is [0, min_spp); a later round takes batch samples (batch 0:
 * `done` more, doubling the total), cut at max_spp; *count == 0 when
 * done >= max_spp.  RTW_ERR_INVALID for parameters outside the ranges above
 * or done not a value the schedule reaches (0, or in [min_spp, max_spp]). */
int rtw_adaptive_next_round(const rtw_adaptive_params* adaptive, int done, int* begin, int* count);

/* The adaptive loop.  Round 0 renders [0, min_spp) of every pixel; each later
 * round selects the active pixels under (floor, target_rel, max_spp) and
 * renders the schedule's next range of them; it ends when the list is empty
 * or max_spp samples are done.  A pixel that drops out never comes back (its
 * moments no longer change), so all active pixels share one sample count.
 * params gives the image, depth, seed and precision (its spp, spp_begin,
 * spp_count and rows are not read).  The three buffers are OVERWRITTEN, not
 * added to; with host buffers the moments, counts and list still stay on the
 * card during the loop and are copied out once.  accum_sq_rgb and counts are
 * required.  out_stats sums the rounds' statistics.  See BIAS above. */
int rtw_render_adaptive(void* scene_handle, const rtw_camera_desc* camera, const rtw_render_params* params,
                        const rtw_adaptive_params* adaptive, double* accum_rgb, double* accum_sq_rgb,
                        uint32_t* counts, rtw_adaptive_result* out_result /* may be NULL */,
                        rtw_stats* out_stats /* may be NULL */);

/* The traversal kernel an active render of this handle (with the scene's own
 * camera) launches now, as rtw_scene_info.kernel names kernels; a render
 * through the wavefront forms reads "k_regen_active + k_segment<...>".
 * precision: RTW_PRECISION_FP64 / RTW_PRECISION_FP32 (rtw_scene_info cannot
 * grow, hence a function of its own). */
int rtw_scene_query_active(void* scene_handle, int precision, char name[128]);

#ifdef __cplusplus
}
#endif

#endif /* RTW_ADAPTIVE_H */
