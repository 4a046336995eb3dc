// rtw_layout.h — what the scene upload (host/scene_layout.cpp) and the kernels
// (rtw_device.h, rtw_fast.h) share: the records of the device scene, their
// tags and limits, and the fp64 vector math the upload evaluates on the host
// with the device's expressions.  Plain C++17 (no HIP header): it compiles
// under g++ and under hipcc's host and device passes.
#pragma once
#include <stdint.h>
#include <cmath>
#include "rtw_gpu.h"
#include "rtw_div.h"

namespace rtwd {

// ------------------------------------------------------------------ vec3
struct d3 {
    double x, y, z;
};
RTW_HD d3 mk(double x, double y, double z) { return d3{x, y, z}; }
RTW_HD d3 operator+(d3 a, d3 b) { return d3{a.x + b.x, a.y + b.y, a.z + b.z}; }
RTW_HD d3 operator-(d3 a, d3 b) { return d3{a.x - b.x, a.y - b.y, a.z - b.z}; }
RTW_HD d3 operator*(d3 a, d3 b) { return d3{a.x * b.x, a.y * b.y, a.z * b.z}; }
RTW_HD d3 operator*(d3 a, double s) { return d3{a.x * s, a.y * s, a.z * s}; }
// d3 / double (vec3.h operator/): three IEEE divisions.  (Sharing one
// reciprocal behind a range vote measured T -3.3 %: EXPERIMENTS.md.)
RTW_HD d3 operator/(d3 a, double s) { return d3{a.x / s, a.y / s, a.z / s}; }
RTW_HD d3 operator-(d3 a) { return d3{-a.x, -a.y, -a.z}; }
RTW_HD double len2(d3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
RTW_HD double len(d3 a) { return __builtin_sqrt(len2(a)); }
RTW_HD d3 cross(d3 a, d3 b) {  // vec3.h:54-59
    return d3{a.y * b.z - a.z * b.y, -(a.x * b.z - a.z * b.x), a.x * b.y - a.y * b.x};
}
// (the compiler's sqrt: in onb_from_w a wave-uniform branch inside the
// frame's normalizations turned the onb into a scratch object)
RTW_HD d3 normalize_b(d3 v) { return v / len(v); }

// ------------------------------------------------------------------ onb
struct onb {
    d3 u, v, w;
};
// Vectors whose length is known to be about 1 are normalised
// with rtw_div.h's bare sqrt sequence (sqrt_core: the compiler's sqrt for x
// >= 2^-766, without its range and class handling -- no branch, no vote):
// the second axis of every frame (cross(w, a) with w unit and |w.x| <= 0.9
// when a = x, so |.|^2 >= 0.19 -- or >= 0.81), and frame_w of a lambertian
// surface's normal (hit_record: (p - c) / r of a sphere, an axis normal,
// rotated orthogonally; surf_frame::unit, a constant where shade_core builds
// the frame -- a per-lane choice of the two forms made the frame a scratch
// object).  A non-finite vector gives NaN either way.  T +0.25 %, C3 +0.25 %
// (profiles/r05/ab_r5r_sqrt_unit.log).
RTW_HD d3 normalize_unit(d3 v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return v / sqrt_core(len2(v));
#else
    return normalize_b(v);
#endif
}
RTW_HD onb onb_from_w(d3 n) {  // onb.h:32-38
    onb b;
    b.w = normalize_b(n);
    const d3 a = (fabs(b.w.x) > 0.9) ? d3{0, 1, 0} : d3{1, 0, 0};
    b.v = normalize_unit(cross(b.w, a));
    b.u = cross(b.w, b.v);
    return b;
}

// ------------------------------------------------------------------ scene
// entry >= 0: one world-list entry; WORLD_RUN_PLAIN: consecutive plain
// entries (one untransformed group each) scanned as their contiguous prims;
// WORLD_RUN_YSPHERES: the same, all spheres for ysphere_scan.
enum : int { WORLD_RUN_PLAIN = -1, WORLD_RUN_YSPHERES = -2 };
struct bvh_node32;
// Device BVH node format (rtw_scene_upload writes it, node_at reads it):
// 32-B nodes with fp32 bounds.  (16-B fp16 nodes, twice the nodes per LDS
// packet, measured C5 -6 %, C3 -9 %: the packet already holds every node of
// C3 and C5 and the fp16 decode costs more; EXPERIMENTS.md.)
using node_store = bvh_node32;
struct world_run {
    int32_t entry, first_prim, n_prims, movers;  // movers: the prims hold DP_MOVING_COMMON*
};
// Device form of a world-list entry (rtw_entry, built by the upload): the
// header alone, its transform ops in one pool (scene::ops) -- 48 B instead of
// the ABI's 312, so a scene's entries stay small in the LDS shading prefix
// whatever RTW_MAX_OPS is, and op chains have no length limit here.
struct dev_entry {
    int32_t kind, first_prim, n_prims, n_ops;
    int32_t first_op;     // ops [first_op, first_op + n_ops) of scene::ops, outermost first
    int32_t phase_material, bvh_root;
    int32_t n_outer_ops;  // MEDIUM: ops enclosing the medium (rtw_entry::n_outer_ops)
    int32_t movers;       // the group holds DP_MOVING_COMMON* spheres
    int32_t pad;
    double neg_inv_density;  // MEDIUM: -(1 / density) (hittable.h:451), IEEE on the host at upload
};
struct dev_op {
    int32_t type, pad;
    double p[3];
};

// Device primitive types.  rtw_scene_upload rewrites the sphere records it
// copies to the GPU (the caller's rtw_scene_desc is untouched), each value
// with the reference's own expression, evaluated once instead of per test:
//   spheres:         p[9] = radius * radius                  (sphere.h:52)
//   moving spheres:  p[4..6] = center1 - center0, p[8] = time1 - time0
//                                                             (sphere.h:24)
// and moving spheres whose (time0, time1) equal the scene's common interval
// (scene::mv_t0 / mv_den) get DP_MOVING_COMMON: their fraction
// (time - time0) / (time1 - time0) is computed once per walk (motion_frac)
// instead of once per sphere.  DP_MOVING_COMMON_Y: in addition
// center1 - center0 = (0, dy, 0) and center0.x, center0.z are nonzero, so
// center0.x + 0 * f == center0.x exactly (f is finite: upload checks the
// interval) and only y moves.
enum : int { DP_MOVING_COMMON = 5, DP_MOVING_COMMON_Y = 6 };
RTW_HD bool is_sphere(int type) { return type < RTW_PRIM_RECT_XY || type > RTW_PRIM_RECT_YZ; }

RTW_HD d3 rect_normal(int type) {
    return type == RTW_PRIM_RECT_XY ? d3{0, 0, 1} : (type == RTW_PRIM_RECT_XZ ? d3{0, 1, 0} : d3{1, 0, 0});
}

// ysphere_scan's fp32 records in flight ahead of the filtered one (the
// upload leaves kYsAhead + 2 spare records after the last prim's).  Only the
// layout (host/scene_layout.cpp) reads it: a variant build that sets
// RTW_YS_AHEAD passes it to the host sources (build_variant_library, host=True).
#ifndef RTW_YS_AHEAD
#define RTW_YS_AHEAD 4
#endif
constexpr int kYsAhead = RTW_YS_AHEAD;

// Device BVH node (rtw_scene_upload): the builder's padded fp64 bounds
// rounded OUTWARD to fp32, children / leaf range in two ints.  32 B instead
// of rtw_bvh_node's 64, and the slab test (slab32) runs in fp32 (twice the
// fp64 rate on gfx950).
struct bvh_node32 {
    float lo[3], hi[3];
    int32_t a;  // inner: left child; leaf: first item
    int32_t b;  // inner: right child | pad << 28 (push_children); leaf: -count
};

// Entries of a BVH traversal stack (local_stack).  Nested walks (a group BVH
// inside a world-BVH leaf) share one stack above the outer walk's entries;
// the host checks at upload that the deepest nesting fits (rtw_scene_upload).
constexpr int kStack = 48;

}  // namespace rtwd

namespace rtwf {

// The fp32 mirror's records (rtw_fast.h).
// p: sphere  c0 xyz, r, c1 - c0 xyz, time0, 1 / (time1 - time0), r^2
//    rect    lo_a, hi_a, lo_b, hi_b, k
struct prim32 {
    int32_t type, material, flip, entry;
    float p[10];
    int32_t pad[2];
};  // 64 B
struct ent32 {
    int32_t kind, first_prim, n_prims, n_ops, first_op, phase_material, bvh_root, n_outer_ops;
    float neg_inv_density;  // -1 / density (hittable.h:450)
    int32_t pad[3];
};  // 48 B
struct op32 {
    int32_t type;
    float p[3];
};  // 16 B
struct mat32 {
    int32_t type, texture;
    float albedo[3], fuzz, ref_idx, inv_ref_idx, r0;
    int32_t pad;
};  // 40 B
struct tex32 {
    int32_t type, odd, even;  // RTW_TEX_IMAGE: odd / even = the image's nx / ny
    float scale;
    float color[3];
    int32_t offset;  // RTW_TEX_IMAGE: byte offset of its first texel in fscene::texels
};  // 32 B

}  // namespace rtwf
