// rtw_select.h — which kernel a render runs: the template arguments the
// kernels are specialised by, the instantiations that exist, and the choice
// among them.  Plain C++17 (no HIP): rtw_kernels.hip builds its launch tables
// from the lists here, and tests/cpp/select_check.cpp walks the choice on the
// CPU.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <string>

namespace rtwd {

// Scene features a traversal kernel is specialised for.
// F_YSPH: the world list holds y-sphere runs (ysphere_scan); without it such
// runs take group_scan (same results), which keeps the prefilter's code and
// registers out of the kernels of other scenes (Cornell).
// F_STATIC: no moving spheres, so a ray's time is never read (sphere.h:22-25
// is its only reader); the persistent kernels then keep no time per path
// (the camera still draws it: the RNG sequence is the reference's).
// F_LIGHTS: the scene has lights, so every lambertian bounce samples the
// mixture pdf (RayTracingWeekend.cpp:112-132) and the lights-free branch is
// compiled out.
// F_BLACK: black background and colour rendering (RayTracingWeekend.cpp:
// 135-159): a miss emits 0 and the normal-visualisation branch is compiled out.
// F_NOLIGHTS: the scene has no lights, so the mixture-pdf branch of the
// lambertian bounce is compiled out instead.
enum : int { F_MEDIA = 1, F_WBVH = 2, F_GBVH = 4, F_YSPH = 8, F_STATIC = 16, F_LIGHTS = 32, F_BLACK = 64,
             F_NOLIGHTS = 128,
             // every camera ray of the render starts at the camera's origin (a
             // pinhole camera, lens_radius 0, whose origin has no zero
             // coordinate: origin + offset is then exactly origin, camera.h:48)
             F_PIN = 256,
             // the render lists its pixels (rtw_adaptive.h): the camera sample's
             // pixel is read from the active list (rtw_kernels.hip sample_coords).
             // Only the instantiations of the active lists below carry the bit;
             // it is free in the FF_* range of the fp32 kernels too.
             F_ACTIVE = 512,
             // the paths start from rays the caller supplies (rtw_radiance.h): a fresh
             // path's ray and stream come from the job's ray records, not the camera
             // (rtw_kernels.hip ray_sample).  Only kPersistRaysList's rows carry the bit.
             F_RAYS = 1024 };
// fp32 kernels for scenes without a noise texture (F bit, fast kernels only):
// the marble texture compiled out of shading (rtw_fast.h texture_value)
constexpr int FF_NONOISE = 1 << 12;
// ... and for scenes with image textures: the texel lookup and the surface
// coordinates compiled in (rtw_fast.h image_value); without this bit no fp32
// kernel carries them
constexpr int FF_IMAGE = 1 << 13;

// Shade-kernel specialisation by the scene's material / texture set.
// SF_ALL: every material and every texture but the image texture (its value
// is part of the kernels' names); SF_IMAGE: the scene holds image textures,
// so shading forms surface coordinates (u, v) where a texture walk reaches
// one -- only kernels compiled with this bit carry that code.
enum : int { SF_NOISE = 1, SF_CHECKER = 2, SF_METAL = 4, SF_DIEL = 8, SF_ISO = 16, SF_ALL = 31, SF_IMAGE = 32 };

// Shade kernels are instantiated for a few material/texture sets; a scene
// runs the smallest instantiated superset of its own set.
constexpr int SF_NOCHECKER = SF_ALL & ~SF_CHECKER;  // the Book-2 set: noise, metal, glass, media
// Scenes with image textures (SF_IMAGE) run one set: everything.  A scene
// without them matches one of the sets before it, as it always did.
constexpr int SF_IMG_ALL = SF_ALL | SF_IMAGE;
constexpr int kShadeMasks[] = {SF_DIEL, SF_METAL | SF_DIEL, SF_NOISE, SF_NOCHECKER, SF_ALL, SF_IMG_ALL};

constexpr uint32_t kShadeLdsMax = 40 * 1024;

inline int pick_shade_mask(int mask) {
    for (int cand : kShadeMasks)
        if ((mask & ~cand) == 0) return cand;
    return SF_IMG_ALL;
}

constexpr int kLdsStack = 16;  // LDS stack entries per lane

// Kernel names as rocprofv3 demangles them ("k_persist_sort<112, 8, true>"),
// for rtw_scene_query and the bench's PMC bookkeeping.
inline std::string kname(const char* k, int f, int m, int lds = -1, int lst = -1) {
    std::string s = std::string(k) + "<" + std::to_string(f);
    if (m >= 0) s += ", " + std::to_string(m);
    if (lds >= 0) s += lds ? ", true" : ", false";
    if (lst >= 0) s += lst ? ", true" : ", false";
    return s + ">";
}

}  // namespace rtwd

namespace rtwf {

// LDS stack entries per lane of the fp32 kernels.  The media kernel's walks
// are group walks from an empty stack (a scene with media has no world BVH),
// which hold at most D entries for a tree of depth D (select_fp32:
// group_depth), so 12 entries serve Book 2's trees (depths 10 and 12) where
// the general bound (world + group depth + 2) asks for 16.  The 8 KB this
// frees per workgroup grows the node packet from 1 534 to all 1 668 of Book
// 2's nodes at two 1 024-thread workgroups per CU, and every node is then an
// LDS read (node_at<PALL>): C5 fp32 32-spp slice 856 vs 828 Msamples/s
// (+3.4 %, profiles/r06/ab_r6o_C5f.log; bit-identical, parity_r6o_mstack.log).
constexpr int kMediaStack = 12;
constexpr int fast_stack(int F) { return (F & rtwd::F_MEDIA) ? kMediaStack : rtwd::kLdsStack; }

}  // namespace rtwf

namespace rtwd {

// ---- the instantiations ----------------------------------------------------
// One entry per compiled kernel: its template arguments <f, m, l> (the fp32
// families have no material set: m = -1, and l is k_fast's LDS-stack flag).
// rtw_kernels.hip instantiates exactly these (one launch-table row each).
struct inst {
    int f, m;
    bool l;
};
constexpr bool operator==(const inst& a, const inst& b) { return a.f == b.f && a.m == b.m && a.l == b.l; }

template <class L, class X>
constexpr int index_of(const L& list, const X& x) {
    for (size_t k = 0; k < list.size(); ++k)
        if (list[k] == x) return (int)k;
    return -1;
}

// k_persist_sort<f, m, l>, k_persist<f, m, l, false> and k_persist<f, m, l,
// true> (LDS traversal stacks) of every entry.
#ifndef RTW_SUBSET
constexpr std::array kPersistList{
    // scenes with image textures: list scenes (y-sphere runs take
    // group_scan: same results) and a world BVH, every material and texture,
    // scene data through the caches
    inst{0, SF_IMG_ALL, false}, inst{F_WBVH, SF_IMG_ALL, false},
    // the pinhole form (F_PIN: camera batches without origins, a larger node
    // packet).  Measured (1 MI355X, A/B, profiles/r04/ab_pin_quad_boxrcp.log):
    // C5 slice 656.1 vs 644.8 Msamples/s (the packet then holds all 1 668 of
    // Book 2's nodes); C3 2 918 vs 2 933 (its 969 nodes fit already): the
    // Book-2 kernel only.
    inst{F_MEDIA | F_GBVH | F_LIGHTS | F_BLACK | F_PIN, SF_NOCHECKER, false},
    // specialised: small list scenes whose shading data fit in LDS, and the
    // lambertian / metal / dielectric sets of the Book-1 scene, flat or BVH
    inst{F_STATIC | F_LIGHTS | F_BLACK, SF_DIEL, true}, inst{F_STATIC | F_LIGHTS, SF_DIEL, true},
    inst{0, SF_DIEL, true}, inst{0, SF_METAL | SF_DIEL, true}, inst{0, SF_ALL, true},
    inst{0, SF_METAL | SF_DIEL, false}, inst{F_YSPH | F_NOLIGHTS, SF_METAL | SF_DIEL, false},
    inst{F_YSPH, SF_METAL | SF_DIEL, false}, inst{F_WBVH | F_NOLIGHTS, SF_METAL | SF_DIEL, false},
    inst{F_WBVH, SF_METAL | SF_DIEL, false},
    // media scenes without checker textures (Book 2): the checker's sines
    // and texture recursion compiled out halves the kernel's SGPR spills
    inst{F_MEDIA | F_GBVH | F_LIGHTS | F_BLACK, SF_NOCHECKER, false}, inst{F_MEDIA | F_GBVH, SF_NOCHECKER, false},
    inst{F_MEDIA, SF_NOCHECKER, false},
    // general: every material / texture, scene read through the caches, one
    // instantiation per traversal feature set (a world BVH never holds media)
    inst{0, SF_ALL, false}, inst{F_YSPH, SF_ALL, false}, inst{F_MEDIA, SF_ALL, false}, inst{F_WBVH, SF_ALL, false},
    inst{F_GBVH, SF_ALL, false}, inst{F_YSPH | F_GBVH, SF_ALL, false}, inst{F_MEDIA | F_GBVH, SF_ALL, false},
    inst{F_WBVH | F_GBVH, SF_ALL, false}};
// k_segment<f, m, l>: traversal + shading fused for the common scene shapes
constexpr std::array kSegmentList{inst{0, SF_IMG_ALL, false}, inst{F_WBVH, SF_IMG_ALL, false},
                                  inst{0, SF_DIEL, true},     inst{0, SF_METAL | SF_DIEL, true},
                                  inst{0, SF_ALL, true},      inst{0, SF_ALL, false},
                                  inst{F_WBVH, SF_ALL, false}, inst{F_WBVH, SF_ALL, true}};
// The split pair.  k_shade<m, l> (f = -1: no feature argument) ...
constexpr std::array kShadeList{inst{-1, SF_DIEL, true},
                                inst{-1, SF_DIEL, false},
                                inst{-1, SF_METAL | SF_DIEL, true},
                                inst{-1, SF_METAL | SF_DIEL, false},
                                inst{-1, SF_NOISE, true},
                                inst{-1, SF_NOISE, false},
                                inst{-1, SF_ALL, true},
                                inst{-1, SF_IMG_ALL, false},  // (no LDS form for image scenes: select_fp64)
                                inst{-1, SF_ALL, false}};
// ... and k_intersect<f>: one traversal kernel per scene-feature combination
// (a world BVH never coexists with media: validate_desc)
constexpr std::array kIntersectList{inst{0, -1, false},      inst{F_MEDIA, -1, false},
                                    inst{F_WBVH, -1, false}, inst{F_GBVH, -1, false},
                                    inst{F_MEDIA | F_GBVH, -1, false}, inst{F_WBVH | F_GBVH, -1, false}};
#else
// experiment builds (scripts/ru_kernel.sh): one persistent kernel only
constexpr std::array kPersistList{inst{RTW_SUBSET_F, RTW_SUBSET_M, RTW_SUBSET_L}};
constexpr std::array<inst, 0> kSegmentList{};
constexpr std::array kShadeList{inst{-1, SF_ALL, false}};
constexpr std::array kIntersectList{inst{F_MEDIA | F_GBVH, -1, false}};
#endif
// what a split choice without a row of its own runs: every material with the
// scene read through the caches (no LDS bytes), the traversal of everything
constexpr inst kShadeFallback{-1, SF_ALL, false};
constexpr inst kIntersectFallback{F_MEDIA | F_GBVH, -1, false};
static_assert(index_of(kShadeList, kShadeFallback) >= 0 && index_of(kIntersectList, kIntersectFallback) >= 0,
              "the split pair's fallback rows are instantiated");

// k_fast<f, l> and k_fast_sort<f, l> (l: the scene's fp32 shading data in LDS)
#ifndef RTW_SUBSET_FAST
constexpr std::array kFastList{
    // scenes with image textures: list scenes and world-BVH scenes
    inst{FF_IMAGE, -1, false}, inst{F_WBVH | FF_IMAGE, -1, true}, inst{F_WBVH | FF_IMAGE, -1, false},
    inst{F_WBVH | FF_NONOISE, -1, true},  // random_balls + BVH: no marble texture
    inst{0, -1, false}, inst{F_MEDIA, -1, false}, inst{F_GBVH, -1, false}, inst{F_GBVH, -1, true},
    inst{F_WBVH, -1, false}, inst{F_WBVH, -1, true}, inst{F_WBVH | F_GBVH, -1, false},
    inst{F_WBVH | F_GBVH, -1, true}, inst{F_MEDIA | F_GBVH, -1, false}, inst{F_MEDIA | F_GBVH, -1, true}};
constexpr std::array kFastSortList{inst{FF_NONOISE, -1, true}, inst{FF_NONOISE, -1, false}, inst{F_MEDIA, -1, true},
                                   inst{F_MEDIA, -1, false},   inst{0, -1, true},           inst{0, -1, false}};
constexpr inst kFastFallback{F_MEDIA | F_GBVH, -1, false};  // of a feature set without a row
#elif defined(RTW_SUBSET_FAST_F)  // experiment builds: one BVH kernel k_fast<RTW_SUBSET_FAST_F, true>
constexpr std::array kFastList{inst{RTW_SUBSET_FAST_F, -1, true}};
constexpr std::array<inst, 0> kFastSortList{};
constexpr inst kFastFallback = kFastList[0];
#else  // ... or the list scenes' fp32 kernel and random_balls + BVH's
constexpr std::array kFastList{inst{F_WBVH | FF_NONOISE, -1, true}};
constexpr std::array kFastSortList{inst{FF_NONOISE, -1, true}};
constexpr inst kFastFallback = kFastList[0];
#endif

// ---- the choice --------------------------------------------------------------
enum class kform { persist_sort, persist, persist_lst, segment, split, fast, fast_sort };

// Kernels with the active-pixel indirection (F_ACTIVE, rtw_adaptive.h).  A row
// names ONE kernel form, not the three a kPersistList entry expands to: the
// kernels the built-in scenes select by default, each in the form that scene
// runs.  Every other fp64 render of a pixel list takes the wavefront forms,
// where k_regen_active is the only kernel that makes camera rays.
struct active_inst {
    inst id;
    kform form;
};
constexpr bool operator==(const active_inst& a, const active_inst& b) { return a.id == b.id && a.form == b.form; }
#if !defined(RTW_SUBSET) && !defined(RTW_SUBSET_FAST) && !(defined(RTW_STRICT_RADIANCE) && RTW_STRICT_RADIANCE)
constexpr std::array kPersistActiveList{
    active_inst{{F_STATIC | F_LIGHTS | F_BLACK | F_ACTIVE, SF_DIEL, true}, kform::persist_sort},          // Cornell
    active_inst{{F_YSPH | F_NOLIGHTS | F_ACTIVE, SF_METAL | SF_DIEL, false}, kform::persist_sort},        // random_balls
    active_inst{{F_WBVH | F_NOLIGHTS | F_ACTIVE, SF_METAL | SF_DIEL, false}, kform::persist_lst},         // ... with a BVH
    active_inst{{F_MEDIA | F_GBVH | F_LIGHTS | F_BLACK | F_PIN | F_ACTIVE, SF_NOCHECKER, false}, kform::persist_lst}};  // Book 2 with BVHs
// fp32 is always persistent: the built-in scenes' rows, then one general
// k_fast per traversal walk (rtw_fast.h world_closest has three: world BVH,
// media, list; F_GBVH is tested per entry at run time, the marble texture is
// compiled in), which render every scene of their walk to the same bits.
constexpr std::array kFastActiveList{
    active_inst{{F_WBVH | FF_NONOISE | F_ACTIVE, -1, true}, kform::fast},   // random_balls + BVH
    active_inst{{F_MEDIA | F_GBVH | F_ACTIVE, -1, true}, kform::fast},      // Book 2 with BVHs
    active_inst{{F_GBVH | F_ACTIVE, -1, false}, kform::fast}, active_inst{{F_WBVH | F_GBVH | F_ACTIVE, -1, false}, kform::fast},
    active_inst{{F_MEDIA | F_GBVH | F_ACTIVE, -1, false}, kform::fast}};
constexpr std::array kFastSortActiveList{active_inst{{FF_NONOISE | F_ACTIVE, -1, true}, kform::fast_sort},    // Cornell
                                         active_inst{{FF_NONOISE | F_ACTIVE, -1, false}, kform::fast_sort}};  // random_balls
#else  // experiment builds and the strict-radiance build (which refuses every active call) render whole images only
constexpr std::array<active_inst, 0> kPersistActiveList{}, kFastActiveList{}, kFastSortActiveList{};
#endif

// Kernels whose paths start from caller-supplied rays (F_RAYS, rtw_radiance.h):
// as the active lists, one row per built-in scene in the form it runs by
// default.  No row carries F_PIN: the pinhole batches and the camera-origin
// shortcut assume that every path starts at the camera.  Every other scene
// takes the wavefront forms, refilled by k_regen_rays.
#if !defined(RTW_SUBSET) && !defined(RTW_SUBSET_FAST) && !(defined(RTW_STRICT_RADIANCE) && RTW_STRICT_RADIANCE)
constexpr std::array kPersistRaysList{
    active_inst{{F_STATIC | F_LIGHTS | F_BLACK | F_RAYS, SF_DIEL, true}, kform::persist_sort},          // Cornell
    active_inst{{F_YSPH | F_NOLIGHTS | F_RAYS, SF_METAL | SF_DIEL, false}, kform::persist_sort},        // random_balls
    active_inst{{F_WBVH | F_NOLIGHTS | F_RAYS, SF_METAL | SF_DIEL, false}, kform::persist_lst},         // ... with a BVH
    active_inst{{F_MEDIA | F_GBVH | F_LIGHTS | F_BLACK | F_RAYS, SF_NOCHECKER, false}, kform::persist_lst}};  // Book 2 with BVHs
#else  // (those builds have no radiance queries: the strict build refuses them)
constexpr std::array<active_inst, 0> kPersistRaysList{};
#endif

struct select_env {
    bool wavefront = false;  // RTW_MODE=wavefront: no persistent kernel (fp64)
    bool split = false;      // RTW_SPLIT=1: k_intersect + k_shade, not k_segment
    int sort = -1;           // RTW_SORT: -1 unset, else 0 / 1 forces k_persist / k_persist_sort (A/B, tests)
    bool fast_sort = true;   // RTW_FAST_SORT=0: list scenes take k_fast too (A/B)
};

// What the choice depends on: the uploaded scene, the render's camera, the
// environment and the build.
struct select_in {
    int features = 0;    // F_MEDIA | F_WBVH | F_GBVH
    int shade_mask = 0;  // SF_* set of the scene
    uint32_t shade_bytes = 0, f32_bytes = 0;  // shading data, fp64 and fp32 (LDS when <= kShadeLdsMax)
    int stack_need = 0, group_depth = 0;      // deepest BVH stack / group BVH
    int n_nodes = 0;
    bool ysph = false, static_scene = false, lights = false, black = false, pin = false;
    select_env env;
    bool strict = false;  // RTW_STRICT_RADIANCE build: folds each path's factors in k_persist, never sorts
    bool active = false;  // the render lists its pixels (rtw_render_accumulate_active): select_active
};

struct kernel_choice {
    kform form;
    inst id;  // the template arguments; split: {features, shade set, LDS shading}, the rows by split_resolve
    std::string name;
    bool active = false;  // select_active's: a row of the active lists, or a wavefront form refilled by k_regen_active
    bool rays = false;    // select_rays': a row of kPersistRaysList, or a wavefront form refilled by k_regen_rays
    bool persistent() const { return form != kform::segment && form != kform::split; }
};

// The persistent kernels of an instantiation: material-regrouping
// k_persist_sort for list traversal, plain k_persist under a BVH (measured,
// 1 MI355X: Cornell +14 %, random_balls flat +12 %, Book-2 flat +37 % with
// regrouping; random_balls BVH -8 %, Book-2 BVH -2 %: divergent BVH walks
// dominate there and the per-iteration block barriers cost), with 16-bit LDS
// stacks where the deepest walk and the node ids fit them.
inline kernel_choice persist_choice(const inst& c, const select_in& s) {
    const bool bvh = (c.f & (F_WBVH | F_GBVH)) != 0;
    if (!s.strict && (s.env.sort >= 0 ? s.env.sort != 0 : !bvh))
        return {kform::persist_sort, c, kname("k_persist_sort", c.f, c.m, c.l)};
    const bool lst = bvh && s.stack_need <= kLdsStack && s.n_nodes < 65536;
    return {lst ? kform::persist_lst : kform::persist, c, kname("k_persist", c.f, c.m, c.l, lst)};
}

// fp64.  Persistent unless RTW_MODE=wavefront: the first listed of the
// scene's feature set with the pinhole bit (where the camera allows it), with
// the static / lights / black-background bits, plain, and the general kernel
// (every material, scene data through the caches).  A scene with image
// textures has one candidate.  Without a persistent instantiation: the fused
// k_segment where listed (and RTW_SPLIT is not set), else the split pair,
// which covers everything and is reported as k_intersect<features>.
inline kernel_choice select_active(const select_in& s, bool fp32);  // (a render of a pixel list: below)
inline kernel_choice select_fp64(const select_in& s) {
    if (s.active) return select_active(s, false);
    const int pick = pick_shade_mask(s.shade_mask);
    const bool image = (pick & SF_IMAGE) != 0;  // (no LDS form for image scenes)
    const bool lds = !image && s.shade_bytes <= kShadeLdsMax;
    if (!s.env.wavefront) {
        inst cand[4];
        int n = 0;
        if (image) {
            cand[n++] = {s.features, pick, false};
        } else {
            // world runs are walked: y-sphere scans
            const int f = s.features | (s.ysph && !(s.features & (F_WBVH | F_MEDIA)) ? F_YSPH : 0);
            const int fs = f | (s.static_scene ? F_STATIC : 0) | (s.lights ? F_LIGHTS : F_NOLIGHTS) |
                           (s.black ? F_BLACK : 0);
            if (s.pin) cand[n++] = {fs | F_PIN, pick, lds};
            cand[n++] = {fs, pick, lds};
            cand[n++] = {f, pick, lds};
            cand[n++] = {f, SF_ALL, false};
        }
        for (int k = 0; k < n; ++k)
            if (index_of(kPersistList, cand[k]) >= 0) return persist_choice(cand[k], s);
    }
    const inst seg{s.features, pick, lds};
    if (!s.env.split && index_of(kSegmentList, seg) >= 0)
        return {kform::segment, seg, kname("k_segment", seg.f, seg.m, seg.l)};
    return {kform::split, seg, kname("k_intersect", s.features, -1)};
}

// The rows a split choice launches: kernel_choice::id names {features, shade
// set, LDS shading} as selection wants them, these are the instantiations
// that run.  k_shade stages the scene's shading data in LDS exactly when
// shade.l (the fallback row reads it through the caches).
struct split_rows {
    inst intersect, shade;
};
inline split_rows split_resolve(const inst& id) {
    const inst i{id.f, -1, false}, s{-1, id.m, id.l};
    return {index_of(kIntersectList, i) >= 0 ? i : kIntersectFallback, index_of(kShadeList, s) >= 0 ? s : kShadeFallback};
}

// fp32 fast mode: always persistent (RTW_MODE and RTW_SPLIT do not apply).
// List scenes take the regrouping k_fast_sort, BVH scenes k_fast with LDS
// stacks when the deepest walk fits them; a feature set without a row runs
// kFastFallback.
inline kernel_choice select_fp32(const select_in& s) {
    if (s.active) return select_active(s, true);
    const int f = s.features & (F_MEDIA | F_WBVH | F_GBVH);
    const bool bvh = (f & (F_WBVH | F_GBVH)) != 0;
    kform form = kform::fast;
    inst c{};
    if (s.shade_mask & SF_IMAGE) {
        // k_fast with the lookup compiled in, for list scenes and world-BVH
        // scenes (others are refused before any launch)
        const bool lst = f == F_WBVH && s.stack_need <= rtwf::fast_stack(f) && s.n_nodes < 65536;
        c = f == 0 ? inst{FF_IMAGE, -1, false} : inst{F_WBVH | FF_IMAGE, -1, lst};
    } else if (!bvh && s.env.fast_sort) {
        // Cornell, random_balls: no marble texture
        const int ff = f == F_MEDIA ? F_MEDIA : (s.shade_mask & SF_NOISE) ? 0 : FF_NONOISE;
        form = kform::fast_sort;
        c = {ff, -1, s.f32_bytes <= kShadeLdsMax};
    } else {
        // (media scenes have no world BVH: their walks are group walks from an
        // empty stack, group_depth entries deep)
        const int need = (f & F_MEDIA) ? s.group_depth : s.stack_need;
        const bool lst = bvh && need <= rtwf::fast_stack(f) && s.n_nodes < 65536;
        c = (f == F_WBVH && lst && !(s.shade_mask & SF_NOISE)) ? inst{F_WBVH | FF_NONOISE, -1, true} : inst{f, -1, lst};
    }
    if ((form == kform::fast_sort ? index_of(kFastSortList, c) : index_of(kFastList, c)) < 0)
        form = kform::fast, c = kFastFallback;
    return {form, c, kname(form == kform::fast ? "k_fast" : "k_fast_sort", c.f, -1, c.l)};
}

// A render of a pixel list (s.active).  The kernel the whole-image render of
// the same scene runs, with F_ACTIVE, where the active lists hold it in that
// form.  Else fp64: the wavefront forms as select_fp64 picks them under
// RTW_MODE=wavefront (k_segment where listed and RTW_SPLIT is unset, else the
// split pair), named with the k_regen_active that refills them; fp32: the
// general k_fast of the scene's walk.  fp32 renders of image-texture scenes
// have no active kernel (active_fp32_ok: refused before any launch).
inline bool active_fp32_ok(const select_in& s) { return !(s.shade_mask & SF_IMAGE); }
inline kernel_choice select_active(const select_in& s_in, bool fp32) {
    select_in s = s_in;
    s.active = false;
    const kernel_choice c = fp32 ? select_fp32(s) : select_fp64(s);
    const active_inst want{{c.id.f | F_ACTIVE, c.id.m, c.id.l}, c.form};
    const char* const fam = c.form == kform::persist_sort ? "k_persist_sort"
                            : c.form == kform::fast       ? "k_fast"
                            : c.form == kform::fast_sort  ? "k_fast_sort" : "k_persist";
    const int lst = c.form == kform::persist ? 0 : c.form == kform::persist_lst ? 1 : -1;
    if (fp32) {
        if (c.form == kform::fast_sort ? index_of(kFastSortActiveList, want) >= 0 : index_of(kFastActiveList, want) >= 0)
            return {c.form, want.id, kname(fam, want.id.f, -1, want.id.l), true};
        // (a build with empty active lists has no such row.  The strict build never gets here: its entry points
        // refuse an active call with RTW_ERR_UNSUPPORTED before anything selects.  In an RTW_SUBSET experiment
        // build plan_render answers this choice with "no such instantiation", an error, not a launch.)
        const int f = s.features & (F_MEDIA | F_WBVH | F_GBVH);
        const inst g{((f & F_MEDIA) ? F_MEDIA : (f & F_WBVH) ? F_WBVH : 0) | F_GBVH | F_ACTIVE, -1, false};
        return {kform::fast, g, kname("k_fast", g.f, -1, g.l), true};
    }
    if (!s.strict && c.persistent() && index_of(kPersistActiveList, want) >= 0)
        return {c.form, want.id, kname(fam, want.id.f, want.id.m, want.id.l, lst), true};
    s.env.wavefront = true;
    kernel_choice w = select_fp64(s);
    w.name = "k_regen_active + " + w.name;
    w.active = true;
    return w;
}

// A radiance query (rtw_radiance.h, fp64 only): the paths start from the
// caller's rays.  The kernel a render of the scene with a camera that is no
// pinhole runs (F_PIN never applies: the rays start anywhere), with F_RAYS,
// where kPersistRaysList holds it in that form; else the wavefront forms as
// select_fp64 picks them under RTW_MODE=wavefront, named with the k_regen_rays
// that refills them.  RTW_MODE, RTW_SORT and RTW_SPLIT act as for renders.
inline kernel_choice select_rays(const select_in& s_in) {
    select_in s = s_in;
    s.active = false;
    s.pin = false;
    const kernel_choice c = select_fp64(s);
    const active_inst want{{c.id.f | F_RAYS, c.id.m, c.id.l}, c.form};
    if (!s.strict && c.persistent() && index_of(kPersistRaysList, want) >= 0) {
        const bool sort = c.form == kform::persist_sort;
        return {c.form, want.id, kname(sort ? "k_persist_sort" : "k_persist", want.id.f, want.id.m, want.id.l,
                                       sort ? -1 : c.form == kform::persist_lst ? 1 : 0), false, true};
    }
    s.env.wavefront = true;
    kernel_choice w = select_fp64(s);
    w.name = "k_regen_rays + " + w.name;
    w.rays = true;
    return w;
}

}  // namespace rtwd
