// scene_layout.h — the device scene as the host lays it out: the two blobs
// the kernels read (the fp64 scene and its fp32 mirror), where every array
// sits in them, the scalars of rtwd::scene / rtwf::fscene and the facts that
// steer kernel selection.  rtw_layout_scene is a pure function of the scene
// desc (no HIP, no environment): rtw_scene_upload copies its blobs to the
// card and points the kernels' scene structs into them, and
// tests/cpp/layout_check.cpp checks it on the CPU.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "rtw_gpu.h"
#include "rtw_select.h"

// A 256-byte aligned sub-array of a blob.  bytes == 0: the array is absent
// (a null pointer on the device); off is still its place in the order.
struct layout_span {
    size_t off = 0, bytes = 0;
};

// rtwd::scene's arrays, in blob order.  [0, nodes.off) is what shading reads:
// a small scene's shading data is one contiguous prefix the shade kernels
// stage in LDS.
struct layout_arrays64 {
    layout_span prims, entries, materials, textures, lights, ranvec, perm, media, prim_onb, mat_aux, ops;
    layout_span nodes, items, runs, ysph, boxes;
    layout_span texels;  // the image textures' texels (validate_desc: every image inside them)
};
// rtwf::fscene's own arrays, in blob order (items, runs, media, ysph and
// texels are the fp64 blob's).  [0, end of perm) is everything fp32 shading
// reads: the prefix the regrouping kernel stages in LDS (k_fast_sort).
struct layout_arrays32 {
    layout_span prims, entries, ops, materials, textures, ranvec, frames, lights, perm;
    layout_span nodes, boxes;
};

// The members of rtwd::scene that are not pointers (same names), and the
// three of rtwf::fscene that are not copies of them.
struct layout_scalars {
    double bvh_bound = 0.0;
    float ysb_cx = 0, ysb_cy = 0, ysb_dy = 0, ysb_cz = 0, ysb_r2 = 0;
    int32_t mv_common = 0;
    double mv_t0 = 0.0, mv_den = 1.0;
    int32_t fast_div = 0;
    double light_weight = 0.0;
    int32_t n_entries = 0, n_lights = 0, world_bvh_root = -1, n_nodes = 0, render_type = 0, background = 0;
    int32_t n_media = 0, has_media = 0, n_runs = 0;
    float f_mv_t0 = 0, f_mv_inv_den = 0, f_light_weight = 0;  // fscene::mv_t0, mv_inv_den, light_weight
};

// What kernel selection, rtw_scene_query and the render's checks read of an
// uploaded scene.
struct layout_facts {
    int features = 0;    // F_MEDIA | F_WBVH | F_GBVH of the scene
    int shade_mask = 0;  // SF_* material / texture set
    bool ysph = false;   // the world list holds y-sphere runs (F_YSPH kernels)
    int n_runs = 0, n_ysph_runs = 0, n_plain_runs = 0;  // world-list run layout (rtw_scene_query)
    bool movers = false;                                // it holds moving spheres (else F_STATIC kernels)
    int stack_need = 0;                                 // deepest BVH stack a traversal of this scene can use
    int group_depth = 0;                                // depth of its deepest group BVH
    uint32_t shade_bytes = 0;  // bytes of the fp64 blob's shading prefix
    uint32_t f32_bytes = 0;    // bytes of the fp32 blob fp32 shading reads
    int n_nodes = 0;           // device BVH nodes in use
    bool lights = false;       // the scene has lights
    bool black = false;        // black background and colour rendering
    bool desc_pin = false;     // the desc's own camera is a pinhole (F_PIN kernels; rtw_scene_query)
    // BVH boxes of moving spheres cover the desc camera's shutter only
    bool bvh_motion = false;
    double shutter0 = 0.0, shutter1 = 0.0;
};

struct scene_layout {
    std::vector<char> mem64, mem32;  // the blobs (at least 256 bytes each)
    layout_arrays64 at64;
    layout_arrays32 at32;
    layout_scalars s;
    layout_facts facts;
};

// F_PIN applies to a render whose camera makes every ray at its origin: no
// lens, no zero origin coordinate, and finite u, v (a non-finite u or v --
// vup parallel to the view direction makes u = unit_vector(0) = NaN -- gives
// the reference a NaN offset and NaN rays, camera.h:36-50)
inline bool camera_is_pinhole(const rtw_camera_desc& c) {
    bool uv = true;
    for (int k = 0; k < 3; ++k) uv = uv && std::isfinite(c.u[k]) && std::isfinite(c.v[k]);
    return c.lens_radius == 0.0 && c.origin[0] != 0.0 && c.origin[1] != 0.0 && c.origin[2] != 0.0 && uv;
}

// Lays out a validated desc.  box_table: build the box-plane table (the
// caller's RTW_BOX_TABLE; false: no table, for tests of the rect path).
// RTW_OK, or rtw_fail's code with the reason: a BVH too deep for the
// traversal stack (RTW_ERR_UNSUPPORTED), a world-BVH item out of range or
// box planes whose fp32 rects differ (RTW_ERR_INVALID).
int rtw_layout_scene(const rtw_scene_desc* d, bool box_table, scene_layout* out);

// What selection reads of a laid-out scene (the environment and the build's
// strictness are the caller's); pin: the render's camera is a pinhole.
rtwd::select_in rtw_layout_select_in(const layout_facts& f, bool pin);
