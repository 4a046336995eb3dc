/*
 * rtw_denoise.h — an edge-aware denoiser for the MI355X path tracer: per-pixel
 * first-hit feature sums (albedo, normal, inverse depth, coverage) and the
 * variance-guided edge-avoiding a-trous wavelet filter of SVGF's spatial pass
 * (Dammertz et al. 2010, Schied et al. 2017) on the raw moments of
 * rtw_noise.h.  An addition to rtw_adaptive.h (same library, same conventions,
 * same RTW_ABI_VERSION: new symbols only, no struct of the other headers
 * changes).
 *
 * KNOWN LIMIT.  The features are those of the FIRST hit of a camera sample.
 * What is seen in a mirror or through glass carries the mirror's or the glass's
 * features, so reflections and refractions are smoothed like a flat surface,
 * and a caustic is noise to this filter.
 *
 * ---- features ----------------------------------------------------------------
 * features[(j*nx + i)*8 + k], eight raw sums per pixel (64 bytes, interleaved),
 * each the sum over the pixel's camera samples, in increasing sample order, of
 *   k = 0..2  the albedo of the first hit: the texture value at the hit for a
 *             lambertian or isotropic material, the emit texture's value for a
 *             diffuse light, a metal's albedo, (1,1,1) for a dielectric; on a
 *             miss the background colour color() returns
 *   k = 3..5  the hit record's normal, as Normal mode shows it (a medium's is
 *             (1,0,0)); 0 on a miss
 *   k = 6     1.0 / t, t the hit's ray parameter (IEEE division); 0 on a miss
 *   k = 7     1.0 on a hit, 0.0 on a miss (coverage)
 *
 * ---- the filter, operation by operation ----------------------------------------
 * All arithmetic is IEEE double, in the order written, without fused
 * multiply-add; the host function and the kernels evaluate the same functions
 * (csrc/host/denoise.h), so rtw_denoise_device returns rtw_denoise's bits.
 *
 * PREPARE, per pixel p with n = counts[p] (or the uniform n) samples, S1 / S2
 * its raw moments, f its eight feature sums and fs = feature_spp:
 *   m_c  = S1_c / n                                            per channel c
 *   v_c  = (S2_c - S1_c * m_c) / (n - 1); if (v_c < 0) v_c = 0; v_c = v_c / n
 *   a_c  = f_c / fs + eps_a     N = (f_3, f_4, f_5) / fs   d = f_6 / fs   cov = f_7 / fs
 *   len  = sqrt((N_x*N_x + N_y*N_y) + N_z*N_z); if (len > 0) N = N / len
 *   c_c  = m_c / a_c            v_c = v_c / (a_c * a_c)        demodulation
 *   l    = ((c_r + c_g) + c_b) / 3     lv = ((v_r + v_g) + v_b) / 9
 * p is VALID iff n >= 2, its six moments and eight feature sums are finite and
 * every a_c > 0.  A pixel that is not valid is passed through (out = m, or NaN
 * without samples; variance NaN) and is never a tap of another pixel.
 *
 * ITERATE, k = 0 .. iterations-1 with step = 2^k, for every valid p = (i, j):
 *   g    = sum(wg * lv_q) / sum(wg) over the valid pixels q of the 3x3
 *          neighbourhood of p inside the image (dy outer, dx inner, -1..1)
 *          with |cov_p - cov_q| <= 0.5 and wn(p, q) > 0 (below: across a
 *          geometric edge neither colour nor variance counts),
 *          wg = (1,2,1)[dy+1] * (1,2,1)[dx+1]; lv of this iteration's input
 *   den  = sigma_l * sqrt(g) + 1e-12
 *   for dy = -2..2 (outer), dx = -2..2 (inner), q = (i + dx*step, j + dy*step),
 *   skipping q outside the image, q not valid and |cov_p - cov_q| > 0.5:
 *     x_l = |l_p - l_q| / den
 *     x_z = |d_p - d_q| / (sigma_z * (d_p + d_q) + 1e-12)
 *     wn  = pow2k(max(0, (N_p.x*N_q.x + N_p.y*N_q.y) + N_p.z*N_q.z), normal_power_log2)
 *           when both normals are non-zero, 1 when both are zero, 0 otherwise
 *     w   = (h[dy+2] * h[dx+2]) * exp_neg(x_l + x_z) * wn,  h = (1/16, 1/4, 3/8, 1/4, 1/16)
 *     if (w > 0):  sw = sw + w;  sc_c = sc_c + w * c_q,c;  sv_c = sv_c + (w * w) * v_q,c
 *   c'_c = sc_c / sw    v'_c = sv_c / (sw * sw)    l', lv' from them as above
 * pow2k(x, k) is x after k squarings; exp_neg(x) is exp(-x) for x <= 64 and 0
 * above (csrc/rtw_math.h: a tap 2^-92 of the centre's cannot change a double
 * mean, and weights that far down would only amplify last-bit differences of
 * g).  The centre tap has w > 0, so sw > 0.
 *
 * FINISH: out_c = c_c * a_c, out_var_c = v_c * (a_c * a_c).
 * iterations == 0: out = m bit for bit and out_var = the v_c of the first
 * PREPARE line (no demodulation; the features are not read).
 *
 * out_var is the variance the filter propagates assuming independent taps.
 * That holds for the first pass; later passes read neighbours that share
 * inputs, so it then UNDERESTIMATES (as SVGF's does), which also makes the
 * luminance weight stricter pass by pass.
 */
#ifndef RTW_DENOISE_H
#define RTW_DENOISE_H

#include "rtw_adaptive.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_FEATURE_CHANNELS 8

/* ADD the first-hit feature sums (above) of the samples and rows params
 * selects into features[nx*ny*8]: for sample s of pixel p exactly the camera
 * ray rtw_render_accumulate traces (the same rtw_path_seed stream, jitter, lens
 * and time draws), one world closest-hit query (a medium's free-flight draw
 * included).  Each pixel's sums continue from the buffer's values in increasing
 * sample order, so sample ranges and row shards add up to the bits of one
 * call.  params->accum_on_device is as in rtw_render_accumulate; fp64 only:
 * precision and max_depth are not read (a Normal-mode scene gives the same
 * features as a Shaded one).  out_stats: samples, segments (one per sample)
 * and ms_total.  RTW_ERR_UNSUPPORTED in the strict-radiance build. */
int rtw_render_features(void* scene_handle, const rtw_camera_desc* camera, const rtw_render_params* params,
                        double* features, rtw_stats* out_stats /* may be NULL */);

/* The kernel rtw_render_features launches for this handle ("k_features<F>"),
 * as rtw_scene_query_active names kernels. */
int rtw_scene_query_features(void* scene_handle, char name[128]);

typedef struct rtw_denoise_params {
    double sigma_l;            /* luminance edge-stopping, in standard deviations (> 0)  */
    double sigma_z;            /* relative inverse-depth edge-stopping (> 0)             */
    double eps_a;              /* added to the albedo before demodulation (> 0)          */
    int32_t iterations;        /* a-trous passes, 0..8; pass k has step 2^k             */
    int32_t normal_power_log2; /* the normal weight is cos^(2^this), 0..16             */
} rtw_denoise_params; /* 32 bytes */

/* The defaults: iterations 5, sigma_l 4, normal_power_log2 7 (cos^128) from
 * the SVGF paper; sigma_z 0.1 and eps_a 1e-2 by judgment (inverse depths
 * within 10 % of their sum, an albedo floor of 1 % keeps black surfaces
 * finite); the end-to-end test (tests/test_gpu_denoise.py) passes with them,
 * profiles/denoise/results.txt has its figures. */
void rtw_denoise_default_params(rtw_denoise_params* out);

/* The filter on host buffers: moments of nx*ny*3 doubles, counts[nx*ny] (NULL:
 * every pixel has n samples, n >= 2), the feature sums of feature_spp >= 1
 * samples per pixel; out_rgb[nx*ny*3] the denoised linear mean, out_var
 * (may be NULL) the propagated variance.  RTW_ERR_INVALID: a null buffer or
 * params, nx or ny <= 0, n < 2 without counts, feature_spp < 1, iterations
 * outside [0, 8], normal_power_log2 outside [0, 16], a sigma or eps_a <= 0 or
 * NaN, an output overlapping any other buffer. */
int rtw_denoise(const double* accum_rgb, const double* accum_sq_rgb, const uint32_t* counts /* may be NULL */, int n,
                const double* features, int feature_spp, int nx, int ny, const rtw_denoise_params* params,
                double* out_rgb, double* out_var /* may be NULL */);

/* The same on the GPU for device buffers of the handle's device, bit for bit.
 * Scratch comes from the handle; stream-ordered after the handle's renders;
 * returns when the outputs are written. */
int rtw_denoise_device(void* scene_handle, const double* accum_dev, const double* accum_sq_dev,
                       const uint32_t* counts_dev /* may be NULL */, int n, const double* features_dev, int feature_spp,
                       int nx, int ny, const rtw_denoise_params* params, double* out_dev,
                       double* out_var_dev /* may be NULL */);

/* canvas = min(sqrt(mean), 1): rtw_finalize_canvas without the division, for
 * the filter's output. */
int rtw_finalize_canvas_mean(const double* mean_rgb, int nx, int ny, double* canvas);
int rtw_finalize_canvas_mean_device(void* scene_handle, const double* mean_dev, int nx, int ny, double* canvas_dev);

#ifdef __cplusplus
}
#endif

#endif /* RTW_DENOISE_H */
