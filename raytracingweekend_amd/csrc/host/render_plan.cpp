// render_plan.cpp — rtw_plan_call (render_plan.h): plain C++, no HIP.
#include "render_plan.h"
#include <algorithm>
#include <cmath>
#include <string>
#include "rtw_host_util.h"

int rtw_check_sample_range(const rtw_render_params& R, const char* entry, const char* range_prefix, int* spp_count) {
    if (R.nx <= 0 || R.ny <= 0 || R.spp <= 0 || R.spp_begin < 0 || R.spp_begin > R.spp || R.spp_count < 0)
        return rtw_fail(RTW_ERR_INVALID, std::string(entry) + ": bad image / sample parameters");
    *spp_count = R.spp_count ? R.spp_count : R.spp - R.spp_begin;
    if (R.spp_begin + (long long)*spp_count > R.spp)
        return rtw_fail(RTW_ERR_INVALID, std::string(range_prefix) + "sample range exceeds spp");
    return RTW_OK;
}

int rtw_plan_call(const rtw_render_params& R, const rtw_camera_desc& camera, const layout_facts& facts,
                  const void* accum_rgb, const void* accum_sq, size_t budget, int flog_cus, call_plan* out,
                  const call_active* act) {
    call_plan P;
    P.active = act != nullptr;
    if (int rc = rtw_check_sample_range(R, "rtw_render_accumulate", "", &P.spp_count)) return rc;
    if (R.precision != RTW_PRECISION_FP64 && R.precision != RTW_PRECISION_FP32)
        return rtw_fail(RTW_ERR_INVALID, "rtw_render_accumulate: unknown precision");
    P.row_step = R.row_step > 0 ? R.row_step : 1;
    if (R.row_begin < 0 || R.row_begin >= R.ny) return rtw_fail(RTW_ERR_INVALID, "row_begin out of range");
    P.n_rows = (R.ny - R.row_begin + P.row_step - 1) / P.row_step;
    P.npix = (uint64_t)P.n_rows * (uint64_t)R.nx;
    if ((uint64_t)R.nx * R.ny >= (1ull << 32) || P.npix >= (1ull << 31))
        return rtw_fail(RTW_ERR_INVALID, "image too large for 32-bit pixel ids");
    if (act) {
        // the list replaces row sharding: sample ids index it
        if (R.row_begin != 0 || R.row_step > 1)
            return rtw_fail(RTW_ERR_INVALID, "rtw_render_accumulate_active: row_begin / row_step do not apply to a "
                                             "pixel list (row_begin 0, row_step 0 or 1)");
        if (act->n > P.npix)
            return rtw_fail(RTW_ERR_INVALID, "rtw_render_accumulate_active: more active pixels than the image has");
        if (act->n && !act->list) return rtw_fail(RTW_ERR_INVALID, "rtw_render_accumulate_active: null pixel list");
        P.npix = act->n;
    }
    if (facts.bvh_motion && (std::min(camera.time0, camera.time1) < facts.shutter0 ||
                             std::max(camera.time0, camera.time1) > facts.shutter1))
        return rtw_fail(RTW_ERR_INVALID,
                        "rtw_render_accumulate: camera shutter outside the one the scene's BVH was built for "
                        "(moving spheres); flatten the scene with this camera");
    const size_t img_bytes = (size_t)R.nx * R.ny * 24;
    if (accum_sq && rtw_ranges_overlap(accum_rgb, accum_sq, img_bytes))
        return rtw_fail(RTW_ERR_INVALID, "rtw_render_accumulate_moments: accum_rgb and accum_sq_rgb overlap");
    if (act) {
        // (a duplicate in the list or a buffer under another would make the
        // scatter-add a race)
        const struct {
            const void* p;
            size_t bytes;
        } buf[] = {{accum_rgb, img_bytes}, {accum_sq, img_bytes}, {act->counts, img_bytes / 6}, {act->list, act->n * 4}};
        for (int a = 0; a < 4; ++a)
            for (int b = a + 1; b < 4; ++b)
                if (buf[a].p && buf[b].p && buf[a].bytes && buf[b].bytes &&
                    rtw_spans_overlap(buf[a].p, buf[a].bytes, buf[b].p, buf[b].bytes))
                    return rtw_fail(RTW_ERR_INVALID, "rtw_render_accumulate_active: two of accum_rgb, accum_sq_rgb, "
                                                     "counts and the pixel list overlap");
    }

    if (P.spp_count == 0 || R.max_depth <= 0 || P.npix == 0) {
        // color() with depth <= 0 returns 0 (RayTracingWeekend.cpp:47-48):
        // every sample adds zero radiance, the accumulator is unchanged.
        P.noop = true;
        P.samples = (uint64_t)P.spp_count * P.npix;
        *out = P;
        return RTW_OK;
    }
    P.fast = R.precision == RTW_PRECISION_FP32;
    P.pin = camera_is_pinhole(camera);

    // pool and pass sizing: a pass holds whole samples per pixel, at most
    // `budget` samples (but one per pixel at least) and fewer than 2^32
    // (pass-local sample ids are 32-bit)
    P.pool = R.wavefront_paths > 0 ? (uint32_t)R.wavefront_paths : (1u << 21);
    P.pass_spp = std::max<uint64_t>(1, std::min<uint64_t>(P.spp_count, budget / P.npix));
    P.pass_spp = std::min<uint64_t>(P.pass_spp, ((1ull << 32) - 1) / P.npix);
    P.pass_samples = P.pass_spp * P.npix;
    P.pool = (uint32_t)std::min<uint64_t>(P.pool, P.pass_samples);
    P.pool = std::max<uint32_t>(P.pool, 1);

    P.bytes.pool = rtw_paths_bytes(P.pool);
    P.bytes.fresh = rtw_fresh_bytes(P.pool);
    P.bytes.hits = rtw_hits_bytes(P.pool);
    P.hits_id_off = rtw_hits_id_off(P.pool);
    P.bytes.radiance = P.pass_samples * 24;
    P.bytes.run = P.npix * 24;
    P.bytes.run2 = accum_sq ? P.npix * 24 : 0;
    P.bytes.camera = sizeof(rtw_camera_desc) + 2 * sizeof(double);
    P.bytes.staging = R.accum_on_device ? 0 : img_bytes;
    if (act && !R.accum_on_device) {
        P.bytes.list = P.npix * 4;
        P.bytes.counts = act->counts ? img_bytes / 6 : 0;
    }

    // camera_sample<false>'s pinhole test reads lens_radius and the origin; a
    // lens-less camera whose u or v is not finite gets lens_radius NaN in the
    // device copy: rd = NaN * p, so its offset is NaN as the reference's
    // u * rd.x + v * rd.y is (the same all-NaN rays, the same draws), and the
    // shortcut does not apply
    P.cam_dev = camera;
    bool uv = true;
    for (int k = 0; k < 3; ++k) uv = uv && std::isfinite(camera.u[k]) && std::isfinite(camera.v[k]);
    if (!uv && P.cam_dev.lens_radius == 0.0) P.cam_dev.lens_radius = __builtin_nan("");
    if (P.fast) {
        call_cam32& c = P.cam32;
        for (int k = 0; k < 3; ++k) {
            c.origin[k] = (float)camera.origin[k], c.lower_left[k] = (float)camera.lower_left[k];
            c.horizontal[k] = (float)camera.horizontal[k], c.vertical[k] = (float)camera.vertical[k];
            c.u[k] = (float)camera.u[k], c.v[k] = (float)camera.v[k];
        }
        c.time0 = (float)camera.time0, c.dtime = (float)(camera.time1 - camera.time0);
        c.lens_radius = (float)camera.lens_radius;
    }

    P.seed_mix = rtw_splitmix64(R.seed);
    P.cam_pin = P.pin ? 1u : 0u;
    P.div_npix = rtwd::udiv_magic((uint32_t)P.npix);
    P.div_nx = rtwd::udiv_magic((uint32_t)R.nx);
    // a factor log per thread of the largest resident grid (2 048 threads per
    // CU), one 32-B entry per bounce
    P.flog_threads = (uint32_t)flog_cus * 2048u;
    P.bytes.flog = (size_t)P.flog_threads * (size_t)R.max_depth * 32;
    *out = P;
    return RTW_OK;
}

call_pass rtw_plan_pass(const call_plan& P, const rtw_render_params& R, uint64_t done) {
    call_pass p;
    p.spp_pass = (uint32_t)std::min<uint64_t>(P.pass_spp, P.spp_count - done);
    p.total = (uint32_t)(p.spp_pass * P.npix);
    p.div_spp = rtwd::udiv_magic(p.spp_pass);
    p.s_begin = R.spp_begin + (int)done;
    p.fill = std::min<uint32_t>(P.pool, p.total);
    // every iteration retires >= 1 live segment; a pass needs at most
    // total * max_depth / pool + max_depth iterations plus the lag of the
    // status snapshots -- far beyond that the pool is not draining
    p.iter_cap = (uint64_t)p.total * (uint64_t)R.max_depth / p.fill + 4ull * R.max_depth + 64;
    return p;
}
