/*
 * rtw_noise.h — per-pixel noise estimate of the MI355X path tracer: the
 * second moments of a render's samples, the standard-error map they give and
 * its image-wide summary.  An addition to rtw_gpu.h (same conventions, same
 * RTW_ABI_VERSION: new symbols only, no struct of rtw_gpu.h changes).
 *
 * The reference averages subPixelCount samples per pixel
 * (RayTracingWeekend.cpp:235-241) and has no notion of how noisy that mean
 * is.  rtw_render_accumulate_moments() keeps, beside the sum S1 of a pixel's
 * samples, the sum S2 of their squares; both are RAW moments, so they add
 * across calls, sample ranges, row shards and GPUs exactly as the radiance
 * sums do, and a host loop may render batches of samples until
 * rtw_noise_estimate()'s summary reaches a target (rtw_render --noise-target,
 * render.render_to_noise).
 *
 * Per channel, from S1, S2 and the number n >= 2 of samples accumulated, with
 * these IEEE double operations in this order (no fused multiply-add):
 *     m  = S1 / n;
 *     v  = (S2 - S1 * m) / (n - 1);   if (v < 0) v = 0;    cancellation
 *     se = sqrt(v / n);               standard error of the pixel mean
 * and per pixel
 *     rel = (se_r + se_g + se_b) / ((m_r + m_g + m_b) + 3 * floor)
 * (`floor` > 0 keeps black pixels from dominating the relative error).
 */
#ifndef RTW_NOISE_H
#define RTW_NOISE_H

#include "rtw_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rtw_render_accumulate, and additionally ADD per pixel and channel the sum of
 * the squares of the same samples' radiance, in increasing sample order, into
 * accum_sq_rgb (same layout, same host/device rule as accum_rgb:
 * params->accum_on_device covers both).  accum_rgb receives bit for bit what
 * rtw_render_accumulate adds with the same arguments.  Every sample x adds
 * q = q + x*x (one rounded product, one rounded add, x widened to double
 * first in the fp32 fast mode); NaN and Inf propagate.  The two buffers must
 * not overlap: RTW_ERR_INVALID. */
int rtw_render_accumulate_moments(void* scene_handle, const rtw_camera_desc* camera,
                                  const rtw_render_params* params,
                                  double* accum_rgb, double* accum_sq_rgb, rtw_stats* out_stats);

typedef struct rtw_noise_summary {
    uint64_t pixels;     /* pixels that entered the statistics                  */
    uint64_t nonfinite;  /* pixels left out: a non-finite S1 or S2 in any channel */
    double mean_rel;     /* mean over `pixels` of rel_p                          */
    double max_rel;      /* max  over `pixels` of rel_p                          */
    double rms_stderr;   /* sqrt(mean over pixels*3 channels of se^2)            */
} rtw_noise_summary; /* 40 bytes */

/* The standard-error map and its summary from host buffers of nx*ny*3 raw
 * moments of n samples per pixel.  stderr_rgb (may be NULL) receives se per
 * channel, NaN in the three channels of a non-finite pixel; out (may be NULL)
 * the summary, its three doubles 0 when no pixel is finite.  Pixels are
 * summed in index order.  RTW_ERR_INVALID: a null input, nx or ny <= 0,
 * n < 2, floor <= 0 or NaN, or stderr_rgb overlapping an input. */
int rtw_noise_estimate(const double* accum_rgb, const double* accum_sq_rgb, int nx, int ny, int n,
                       double floor, double* stderr_rgb /* may be NULL */, rtw_noise_summary* out /* may be NULL */);

/* The same on the GPU, for device buffers of the handle's device (stream
 * ordered after the handle's renders; returns when stderr_dev and out_host
 * are written).  The map is bit-identical to rtw_noise_estimate's; the
 * summary's doubles are summed per thread, wave and block of a grid that
 * depends on nx*ny only, then over the blocks in block order, without
 * atomics -- a fixed order, so two calls return the same bits, within
 * nx*ny*eps (relative) of the host function's.  RTW_ERR_INVALID also when a
 * buffer is not device or managed memory of the handle's device. */
int rtw_noise_estimate_device(void* scene_handle, const double* accum_dev, const double* accum_sq_dev,
                              int nx, int ny, int n, double floor,
                              double* stderr_dev /* may be NULL */, rtw_noise_summary* out_host /* may be NULL */);

#ifdef __cplusplus
}
#endif

#endif /* RTW_NOISE_H */
