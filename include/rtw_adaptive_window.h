/*
 * rtw_adaptive_window.h — adaptive sampling that judges a pixel on its
 * neighbourhood's noise: a pixel keeps sampling while any pixel of a small
 * window around it is still loud.  An addition to rtw_adaptive.h (same
 * library, same conventions, same RTW_ABI_VERSION: new symbols only, no struct
 * of the other headers changes).
 *
 * ---- the rule, operation by operation ------------------------------------------
 * A pixel's index is p = j*nx + i, as in the accumulators; counts[nx*ny] is the
 * number of samples each pixel has taken.  The WINDOW of p with radius r is
 * every pixel q = (i_q, j_q) with |i_q - i_p| <= r and |j_q - j_p| <= r INSIDE
 * THE IMAGE: it is clipped at the borders, it does not wrap and does not
 * mirror.  Under (floor, target_rel, min_count, max_count, r):
 *
 *   SOURCE(q)         q's six moments are finite, and
 *                     counts[q] < 2  or  rel_q > target_rel,
 *                     rel_q being rtw_noise.h's expression evaluated with
 *                     n = counts[q] (the same operations in the same order: the
 *                     function rtw_adaptive.h's ACTIVE uses).  It depends on
 *                     neither min_count nor max_count: a pixel that took
 *                     max_count samples and is still loud stays a source for
 *                     its neighbours, since it marks a heavy-tailed region.
 *   ELIGIBLE(p)       min_count <= counts[p] < max_count and p's six moments
 *                     are finite.
 *   WINDOW-ACTIVE(p)  ELIGIBLE(p) and some q of p's window is a SOURCE.
 *
 * With r == 0 and min_count == 0 this is exactly rtw_adaptive.h's ACTIVE.  A
 * non-finite pixel is never listed and never a source.  The rule is a maximum
 * over the window (an OR of per-pixel answers), not a pooled variance: it does
 * not depend on the order the window is walked in, so the host and the device
 * give the same list, element for element.
 *
 * ---- the loop --------------------------------------------------------------------
 * rtw_render_adaptive_window is rtw_render_adaptive with this selection: round
 * k >= 1 selects with min_count = done and max_count = max_spp, `done` being
 * the number of samples the still-active pixels have taken.  min_count keeps
 * the loop's invariant: a pixel that dropped out has counts[p] < done and
 * never comes back, even when a neighbour turns loud later, so all listed
 * pixels share one sample range and each pixel's sums stay those of its
 * samples [0, counts[p]).  Hence
 *   - radius == 0 returns rtw_render_adaptive's buffers, counts, result and
 *     statistics bit for bit;
 *   - every pixel takes at least as many samples as under radius 0 with the
 *     same parameters: a pixel's samples depend on (seed, pixel, sample) only,
 *     so while it is active in the radius-0 run it has the same moments here,
 *     is a source itself and therefore active here.
 *
 * BIAS.  rtw_adaptive.h's loop stops a pixel on the variance of its own
 * samples, which biases dark, heavy-tailed pixels LOW: a pixel whose first
 * min_spp samples all miss a rare bright path looks quiet and stops.  The
 * window asks the (2r+1)^2 pixels around it instead, which between them have
 * taken (2r+1)^2 * min_spp samples and are far more likely to have met that
 * path; the pixel then goes on sampling and its mean recovers.  This REDUCES
 * the bias, it does not remove it: a region none of whose pixels met the path
 * still stops, a pixel that dropped out does not come back, and the remedy
 * costs samples (quiet pixels beside loud ones keep sampling; pixels beside a
 * pixel that stays loud at max_spp run to max_spp themselves).  DESIGN.md has
 * what was measured.  The mean of a uniform render has no such bias.
 */
#ifndef RTW_ADAPTIVE_WINDOW_H
#define RTW_ADAPTIVE_WINDOW_H

#include "rtw_adaptive.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_WINDOW_RADIUS_MAX 16

/* The ascending list of the WINDOW-ACTIVE pixels (definition above) of host
 * buffers and its length; active_out holds up to nx*ny entries.
 * RTW_ERR_INVALID: what rtw_adaptive_select refuses, radius outside
 * [0, RTW_WINDOW_RADIUS_MAX], min_count > max_count. */
int rtw_adaptive_select_window(const double* accum_rgb, const double* accum_sq_rgb, const uint32_t* counts, int nx,
                               int ny, double floor, double target_rel, uint32_t min_count, uint32_t max_count,
                               int radius, uint32_t* active_out, uint64_t* n_active_out);

/* The same on the GPU for device buffers of the handle's device; the length
 * goes to host memory.  No atomics: one bit per pixel for SOURCE and for
 * "finite" (a wave's ballot), the window as shifts and ORs of those words,
 * then rtw_adaptive_select_device's count, scan and ordered scatter on grids
 * that depend on (nx, ny) only: the list is rtw_adaptive_select_window's,
 * element for element, and the same bits on every call.  Scratch comes from
 * the handle. */
int rtw_adaptive_select_window_device(void* scene_handle, const double* accum_dev, const double* accum_sq_dev,
                                      const uint32_t* counts_dev, int nx, int ny, double floor, double target_rel,
                                      uint32_t min_count, uint32_t max_count, int radius, uint32_t* active_dev,
                                      uint64_t* n_active_host);

/* The adaptive loop with the window rule (above); every argument but radius is
 * rtw_render_adaptive's.  RTW_ERR_INVALID additionally for radius outside
 * [0, RTW_WINDOW_RADIUS_MAX]; RTW_ERR_UNSUPPORTED in the strict-radiance
 * build.  See BIAS above. */
int rtw_render_adaptive_window(void* scene_handle, const rtw_camera_desc* camera, const rtw_render_params* params,
                               const rtw_adaptive_params* adaptive, int radius, double* accum_rgb,
                               double* accum_sq_rgb, uint32_t* counts, rtw_adaptive_result* out_result /* may be NULL */,
                               rtw_stats* out_stats /* may be NULL */);

#ifdef __cplusplus
}
#endif

#endif /* RTW_ADAPTIVE_WINDOW_H */
