// layout_check.cpp — rtw_layout_scene (csrc/host/scene_layout.cpp) on the CPU.
//
//   layout_check scenes <dir>
//       every built-in scene of the list below, flat and with BVHs: the two
//       blobs written to <dir>/<scene>_<flat|bvh>.mem64 / .mem32 and one line
//       "<scene>/<flat|bvh>\t<json>" with every array's offset (-1: absent),
//       the scalars, the facts, and the kernels select_fp64 / select_fp32
//       choose from those facts under the five environments of
//       scripts/record_scene_query.py (tests/test_scene_layout.py compares
//       them with the recorded files)
//   layout_check cases
//       hand-built descs, the smallest at which each step of the layout can
//       go wrong, against values written out from the formats documented in
//       rtw_layout.h / rtw_device.h; "OK (<n> checks)" or the failed lines
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "rtw_gpu.h"
#include "rtw_layout.h"
#include "rtw_select.h"
#include "scene_layout.h"

using namespace rtwd;

namespace {

int g_checks = 0, g_failed = 0;
#define CHECK(x)                                                          \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(x)) {                                                       \
            ++g_failed;                                                   \
            std::printf("FAILED %s:%d: %s\n", __func__, __LINE__, #x);    \
        }                                                                 \
    } while (0)

// ---------------------------------------------------------------- scenes
long long off_of(const layout_span& a) { return a.bytes ? (long long)a.off : -1; }

void print_select(const layout_facts& f, bool pin) {
    const struct {
        const char* name;
        select_env env;
    } envs[] = {{"default", {}},
                {"wavefront", {true, false, -1, true}},
                {"wavefront_split", {true, true, -1, true}},
                {"sort0", {false, false, 0, true}},
                {"sort1", {false, false, 1, true}}};
    std::printf("\"select\": {");
    for (size_t k = 0; k < 5; ++k) {
        select_in s = rtw_layout_select_in(f, pin);
        s.env = envs[k].env;
        std::printf("%s\"%s\": {\"kernel\": \"%s\", \"kernel_fast\": \"%s\", \"shade_lds_bytes\": %u}", k ? ", " : "",
                    envs[k].name, select_fp64(s).name.c_str(), select_fp32(s).name.c_str(),
                    f.shade_bytes <= kShadeLdsMax ? f.shade_bytes : 0u);
    }
    std::printf("}");
}

bool write_file(const std::string& path, const std::vector<char>& m) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(m.data(), 1, m.size(), f) == m.size();
    return std::fclose(f) == 0 && ok;
}

int dump_scenes(const std::string& dir) {
    const struct {
        const char* name;
        double aspect;
    } scenes[] = {{"book2_final", 1.0}, {"cornell_box", 1.0},  {"dielectric", 2.0},   {"light_sample", 2.0},
                  {"nested", 1.0},      {"nested_plain", 1.0}, {"random_balls", 1.5}, {"textured", 1.0}};
    for (const auto& sc : scenes)
        for (int bvh = 0; bvh < 2; ++bvh) {
            rtw_scene_desc* d = nullptr;
            scene_layout L;
            if (rtw_scene_builtin(sc.name, sc.aspect, bvh, &d) != RTW_OK || rtw_layout_scene(d, true, &L) != RTW_OK) {
                std::fprintf(stderr, "%s: %s\n", sc.name, rtw_last_error());
                return 1;
            }
            const std::string stem = dir + "/" + sc.name + (bvh ? "_bvh" : "_flat");
            if (!write_file(stem + ".mem64", L.mem64) || !write_file(stem + ".mem32", L.mem32)) return 1;
            std::printf("%s/%s\t{", sc.name, bvh ? "bvh" : "flat");
#define O(m, f) std::printf("\"%s\": %lld, ", #f, off_of(L.m.f))
#define I(m, f) std::printf("\"%s\": %lld, ", #f, (long long)L.m.f)
#define D(m, f) std::printf("\"%s\": \"%a\", ", #f, (double)L.m.f)
            std::printf("\"off64\": {");
            O(at64, prims), O(at64, entries), O(at64, materials), O(at64, textures), O(at64, lights), O(at64, ranvec);
            O(at64, perm), O(at64, media), O(at64, prim_onb), O(at64, mat_aux), O(at64, ops), O(at64, nodes);
            O(at64, items), O(at64, runs), O(at64, ysph), O(at64, boxes), O(at64, texels);
            std::printf("\"end\": %zu}, \"off32\": {", L.mem64.size());
            O(at32, prims), O(at32, entries), O(at32, ops), O(at32, materials), O(at32, textures), O(at32, ranvec);
            std::printf("\"frames\": %zu, ", L.at32.frames.off);  // (never null)
            O(at32, lights), O(at32, perm), O(at32, nodes), O(at32, boxes);
            std::printf("\"end\": %zu}, \"scalars\": {", L.mem32.size());
            D(s, bvh_bound), D(s, ysb_cx), D(s, ysb_cy), D(s, ysb_dy), D(s, ysb_cz), D(s, ysb_r2), I(s, mv_common);
            D(s, mv_t0), D(s, mv_den), I(s, fast_div), D(s, light_weight), I(s, n_entries), I(s, n_lights);
            I(s, world_bvh_root), I(s, n_nodes), I(s, render_type), I(s, background), I(s, n_media), I(s, has_media);
            I(s, n_runs), D(s, f_mv_t0), D(s, f_mv_inv_den), D(s, f_light_weight);
            std::printf("\"_\": 0}, \"facts\": {");
            I(facts, features), I(facts, shade_mask), I(facts, ysph), I(facts, n_runs), I(facts, n_ysph_runs);
            I(facts, n_plain_runs), I(facts, movers), I(facts, stack_need), I(facts, group_depth), I(facts, shade_bytes);
            I(facts, f32_bytes), I(facts, desc_pin), I(facts, bvh_motion), D(facts, shutter0), D(facts, shutter1);
            std::printf("\"_\": 0}, ");
#undef O
#undef I
#undef D
            print_select(L.facts, camera_is_pinhole(d->camera));
            std::printf("}\n");
            rtw_scene_desc_free(d);
        }
    return 0;
}

// ----------------------------------------------------------------- cases
// A desc built by hand.
struct hand {
    std::vector<rtw_prim> prims;
    std::vector<rtw_entry> entries;
    std::vector<rtw_material> materials;
    std::vector<rtw_texture> textures;
    std::vector<rtw_light> lights;
    std::vector<rtw_bvh_node> nodes;
    std::vector<int32_t> items, visits;
    std::vector<double> ranvec;
    std::vector<int32_t> perm;
    int world_root = -1;

    rtw_scene_desc desc() const {
        rtw_scene_desc d;
        std::memset(&d, 0, sizeof d);
        d.abi_version = RTW_ABI_VERSION;
        d.n_prims = (int)prims.size(), d.prims = prims.data();
        d.n_entries = (int)entries.size(), d.entries = entries.data();
        d.n_materials = (int)materials.size(), d.materials = materials.data();
        d.n_textures = (int)textures.size(), d.textures = textures.data();
        d.n_lights = (int)lights.size(), d.lights = lights.data();
        d.n_bvh_nodes = (int)nodes.size(), d.bvh_nodes = nodes.data();
        d.n_bvh_items = (int)items.size(), d.bvh_items = items.data();
        d.n_visits = (int)visits.size(), d.visits = visits.data();
        d.world_bvh_root = world_root;
        d.has_perlin = !ranvec.empty(), d.perlin_ranvec = ranvec.data(), d.perlin_perm = perm.data();
        d.camera.origin[0] = d.camera.origin[1] = d.camera.origin[2] = 1.0;
        d.camera.time0 = 0.0, d.camera.time1 = 1.0;
        return d;
    }
    int layout(scene_layout* L, bool box_table = true) const {
        const rtw_scene_desc d = desc();
        return rtw_layout_scene(&d, box_table, L);
    }
    // a group entry over prims [first, first + n), which it takes
    int group(int first, int n, int bvh_root = -1) {
        rtw_entry e;
        std::memset(&e, 0, sizeof e);
        e.kind = RTW_ENTRY_GROUP, e.first_prim = first, e.n_prims = n, e.bvh_root = bvh_root, e.phase_material = -1;
        entries.push_back(e);
        for (int i = first; i < first + n; ++i) prims[i].entry = (int)entries.size() - 1;
        return (int)entries.size() - 1;
    }
    void op(int e, int type, double a = 0, double b = 0, double c = 0) {
        rtw_entry& E = entries[e];
        E.op[E.n_ops] = type;
        E.op_param[E.n_ops][0] = a, E.op_param[E.n_ops][1] = b, E.op_param[E.n_ops][2] = c;
        ++E.n_ops;
    }
    int sphere(double x, double y, double z, double r) {
        rtw_prim q;
        std::memset(&q, 0, sizeof q);
        q.type = RTW_PRIM_SPHERE, q.entry = -1;
        q.p[0] = x, q.p[1] = y, q.p[2] = z, q.p[3] = r;
        prims.push_back(q);
        return (int)prims.size() - 1;
    }
    int mover(double x, double y, double z, double r, double x1, double y1, double z1, double t0, double t1) {
        const int i = sphere(x, y, z, r);
        rtw_prim& q = prims[i];
        q.type = RTW_PRIM_MOVING_SPHERE;
        q.p[4] = x1, q.p[5] = y1, q.p[6] = z1, q.p[7] = t0, q.p[8] = t1;
        return i;
    }
    int rect(int type, double a0, double a1, double b0, double b1, double k, int flip = 0) {
        rtw_prim q;
        std::memset(&q, 0, sizeof q);
        q.type = type, q.entry = -1, q.flip = flip;
        q.p[0] = a0, q.p[1] = a1, q.p[2] = b0, q.p[3] = b1, q.p[4] = k;
        prims.push_back(q);
        return (int)prims.size() - 1;
    }
    // the six rects of a hittable_list box, in its order; the first one's index
    int box(double x0, double x1, double y0, double y1, double z0, double z1) {
        const int i = rect(RTW_PRIM_RECT_XY, x0, x1, y0, y1, z1);
        rect(RTW_PRIM_RECT_XY, x0, x1, y0, y1, z0, 1);
        rect(RTW_PRIM_RECT_XZ, x0, x1, z0, z1, y1);
        rect(RTW_PRIM_RECT_XZ, x0, x1, z0, z1, y0, 1);
        rect(RTW_PRIM_RECT_YZ, y0, y1, z0, z1, x1);
        rect(RTW_PRIM_RECT_YZ, y0, y1, z0, z1, x0, 1);
        return i;
    }
    int leaf(int first_item, int count, double lo = 0, double hi = 1) {
        rtw_bvh_node n;
        std::memset(&n, 0, sizeof n);
        for (int k = 0; k < 3; ++k) n.bmin[k] = lo, n.bmax[k] = hi;
        n.left = first_item, n.count = count;
        nodes.push_back(n);
        return (int)nodes.size() - 1;
    }
    int inner(int left, int right, double lo = 0, double hi = 1) {
        const int i = leaf(left, 0, lo, hi);
        nodes[i].right = right;
        return i;
    }
};

template <class T>
const T* arr(const std::vector<char>& m, const layout_span& a) {
    return reinterpret_cast<const T*>(m.data() + a.off);
}
size_t al(size_t bytes) { return (bytes + 255) & ~size_t(255); }
bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }
bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// 0.7 = 0x1.6666666666666p-1 lies between the floats 0x1.666666p-1 (the
// nearest) and 0x1.666668p-1; 0.1 = 0x1.999999999999ap-4 between
// 0x1.999998p-4 and 0x1.99999ap-4 (the nearest).
void ysphere_runs() {
    hand h;
    h.sphere(1.5, 0.7, -2.0, 0.5);
    h.sphere(3.0, 2.0, 4.0, 1000.0);
    h.sphere(-1.75, 0.5, 7.0, 0.25);
    h.prims[0].p[5] = 9.0;  // (not a sphere's field: a y-sphere run's dy)
    h.group(0, 3);
    scene_layout L;
    CHECK(h.layout(&L) == RTW_OK);
    const world_run* R = arr<world_run>(L.mem64, L.at64.runs);
    CHECK(L.s.n_runs == 1 && L.at64.runs.bytes == sizeof(world_run));
    CHECK(R[0].entry == WORLD_RUN_YSPHERES && R[0].first_prim == 0 && R[0].n_prims == 3 && R[0].movers == 0);
    CHECK(L.facts.ysph && L.facts.n_ysph_runs == 1 && L.facts.n_plain_runs == 0 && L.facts.n_runs == 1);
    const rtw_prim* P = arr<rtw_prim>(L.mem64, L.at64.prims);
    CHECK(P[0].p[5] == 0.0 && P[1].p[5] == 0.0 && P[2].p[5] == 0.0);
    CHECK(P[0].p[9] == 0.25 && P[1].p[9] == 1e6 && P[2].p[9] == 0.0625);
    CHECK(P[0].type == RTW_PRIM_SPHERE);
    // the pair at floats [0, 16): component c of member s at 2c + s
    const float* Y = arr<float>(L.mem64, L.at64.ysph);
    CHECK(L.at64.ysph.bytes == 4 * 8 * (3 + kYsAhead + 2));
    const float inf = INFINITY;
    const float pair[16] = {1.5f, 3.0f, 0x1.666666p-1f, 2.0f, -2.0f, 4.0f, 0.0f, 0.0f, 0.25f, inf, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 16; ++k) CHECK(same(Y[k], pair[k]));
    // the third: a lone plain record {cx, cy, cz, dy, rr} in its own 8 floats
    const float lone[8] = {-1.75f, 0.5f, 7.0f, 0.0f, 0.0625f, 0, 0, 0};
    for (int k = 0; k < 8; ++k) CHECK(same(Y[16 + k], lone[k]));
    for (size_t k = 24; k < L.at64.ysph.bytes / 4; ++k) CHECK(Y[k] == 0.0f);
    // maxima over the filtered spheres only (not the r = 1000 one), rounded up
    CHECK(same(L.s.ysb_cx, 1.75f) && same(L.s.ysb_cy, 0x1.666668p-1f) && same(L.s.ysb_dy, 0.0f));
    CHECK(same(L.s.ysb_cz, 7.0f) && same(L.s.ysb_r2, 0.25f));
    CHECK(L.s.fast_div == 1 && L.s.mv_common == 0 && !L.facts.movers);

    // one sphere at y == 0: the run stays plain, and p[5] is left alone
    h.prims[0].p[1] = 0.0;
    CHECK(h.layout(&L) == RTW_OK);
    R = arr<world_run>(L.mem64, L.at64.runs);
    CHECK(L.s.n_runs == 1 && R[0].entry == WORLD_RUN_PLAIN && R[0].n_prims == 3);
    CHECK(!L.facts.ysph && L.facts.n_plain_runs == 1 && L.facts.n_ysph_runs == 0);
    CHECK(arr<rtw_prim>(L.mem64, L.at64.prims)[0].p[5] == 9.0);
    Y = arr<float>(L.mem64, L.at64.ysph);
    for (size_t k = 0; k < L.at64.ysph.bytes / 4; ++k) CHECK(Y[k] == 0.0f);
    CHECK(L.s.ysb_cx == 0.0f && L.s.ysb_r2 == 0.0f);
}

void movers() {
    hand h;
    h.mover(1, 2, 3, 0.5, 1, 2.5, 3, 0.25, 1.0);   // dc = (0, 0.5, 0): y only
    h.mover(1, 2, 3, 0.5, 2, 2, 3, 0.25, 1.0);     // dc = (1, 0, 0)
    h.mover(0, 2, 3, 0.5, 0, 3, 3, 0.25, 1.0);     // dc = (0, 1, 0) but x == 0
    h.mover(1, 2, 3, 0.5, 1, -2.5, 3, 0.25, 1.0);  // dc = (0, -4.5, 0)
    h.group(0, 4);
    scene_layout L;
    CHECK(h.layout(&L) == RTW_OK);
    const rtw_prim* P = arr<rtw_prim>(L.mem64, L.at64.prims);
    CHECK(P[0].type == DP_MOVING_COMMON_Y && P[1].type == DP_MOVING_COMMON && P[2].type == DP_MOVING_COMMON);
    CHECK(P[3].type == DP_MOVING_COMMON_Y);
    // sphere.h:52 radius * radius; sphere.h:24 center1 - center0, time1 - time0
    CHECK(P[0].p[9] == 0.25 && P[0].p[4] == 0.0 && P[0].p[5] == 0.5 && P[0].p[6] == 0.0 && P[0].p[8] == 0.75);
    CHECK(P[0].p[7] == 0.25 && P[1].p[4] == 1.0 && P[1].p[5] == 0.0 && P[3].p[5] == -4.5);
    CHECK(L.s.mv_common == 1 && L.s.mv_t0 == 0.25 && L.s.mv_den == 0.75 && L.s.fast_div == 1);
    CHECK(same(L.s.f_mv_t0, 0.25f) && same(L.s.f_mv_inv_den, (float)(1.0 / 0.75)));
    CHECK(L.facts.movers && !L.facts.bvh_motion);
    const world_run* R = arr<world_run>(L.mem64, L.at64.runs);
    CHECK(R[0].entry == WORLD_RUN_PLAIN && R[0].movers == 1);  // (not all y-only)
    CHECK(arr<dev_entry>(L.mem64, L.at64.entries)[0].movers == 1);
    // the fp32 mirror: p[8] = 1 / (time1 - time0), from the desc's own values
    const rtwf::prim32* Q = arr<rtwf::prim32>(L.mem32, L.at32.prims);
    CHECK(Q[0].type == RTW_PRIM_MOVING_SPHERE && same(Q[0].p[8], (float)(1.0 / 0.75)) && same(Q[0].p[5], 0.5f));
    CHECK(same(Q[0].p[9], 0.25f) && same(Q[0].p[7], 0.25f));

    // a fifth on another interval keeps its type and ends the shared divisor
    h.mover(1, 2, 3, 0.5, 1, 2.5, 3, 0.0, 2.0);
    h.entries[0].n_prims = 5, h.prims[4].entry = 0;
    CHECK(h.layout(&L) == RTW_OK);
    P = arr<rtw_prim>(L.mem64, L.at64.prims);
    CHECK(P[4].type == RTW_PRIM_MOVING_SPHERE && P[4].p[8] == 2.0 && P[4].p[5] == 0.5 && P[4].p[9] == 0.25);
    CHECK(P[0].type == DP_MOVING_COMMON_Y && L.s.fast_div == 0 && L.s.mv_t0 == 0.25);

    // an interval shorter than 1e-200 never becomes the common one
    hand g;
    g.mover(1, 2, 3, 0.5, 1, 2.5, 3, 0.0, 1e-201);
    g.mover(1, 2, 3, 0.5, 1, 2.5, 3, 0.5, 1.5);
    g.group(0, 2);
    CHECK(g.layout(&L) == RTW_OK);
    P = arr<rtw_prim>(L.mem64, L.at64.prims);
    CHECK(P[0].type == RTW_PRIM_MOVING_SPHERE && P[1].type == DP_MOVING_COMMON_Y);
    CHECK(L.s.mv_common == 1 && L.s.mv_t0 == 0.5 && L.s.mv_den == 1.0 && L.s.fast_div == 0);

    // dc = (-0, dy, -0).  center1 - center0 is -0 only for -0 - +0 (x - x is
    // +0 for every x != 0), and a centre component at 0 is no y-only mover:
    // the deltas keep their sign and the sphere is DP_MOVING_COMMON.  With
    // nonzero x and z (the second sphere) the deltas are +0: y only.
    hand z;
    z.mover(0.0, 2, 0.0, 0.5, -0.0, 3, -0.0, 0.25, 1.0);
    z.mover(-1, 2, -3, 0.5, -1, 3, -3, 0.25, 1.0);
    z.group(0, 2);
    CHECK(z.layout(&L) == RTW_OK);
    P = arr<rtw_prim>(L.mem64, L.at64.prims);
    CHECK(P[0].p[4] == 0.0 && std::signbit(P[0].p[4]) && P[0].p[6] == 0.0 && std::signbit(P[0].p[6]) && P[0].p[5] == 1.0);
    CHECK(P[0].type == DP_MOVING_COMMON && P[1].type == DP_MOVING_COMMON_Y);
    CHECK(same(P[1].p[4], 0.0) && same(P[1].p[6], 0.0) && P[1].p[5] == 1.0 && L.s.fast_div == 1);
}

void runs() {
    hand h;
    h.sphere(0, 1, 0, 1);                        // e0
    h.rect(RTW_PRIM_RECT_XY, 0, 1, 0, 1, 2);     // e1: flip only
    h.sphere(5, 1, 0, 1);                        // e2: rotate_y
    h.sphere(6, 1, 0, 1), h.sphere(7, 1, 0, 1);  // e3: a group BVH
    h.mover(1, 2, 3, 0.5, 2, 2, 3, 0.0, 1.0);    // e4
    h.sphere(8, 0, 0, 1);                        // e5
    h.group(0, 1);
    h.op(h.group(1, 1), RTW_OP_FLIP);
    h.op(h.group(2, 1), RTW_OP_ROTATE_Y, 0.6, 0.8);
    h.items = {3, 4};
    h.group(3, 2, h.leaf(0, 2));
    h.group(5, 1);
    h.group(6, 1);
    scene_layout L;
    CHECK(h.layout(&L) == RTW_OK);
    const world_run* R = arr<world_run>(L.mem64, L.at64.runs);
    CHECK(L.s.n_runs == 4 && L.at64.runs.bytes == 4 * sizeof(world_run));
    CHECK(R[0].entry == WORLD_RUN_PLAIN && R[0].first_prim == 0 && R[0].n_prims == 2 && R[0].movers == 0);
    CHECK(R[1].entry == 2 && R[1].first_prim == 2 && R[1].n_prims == 1);
    CHECK(R[2].entry == 3 && R[2].first_prim == 3 && R[2].n_prims == 2);
    CHECK(R[3].entry == WORLD_RUN_PLAIN && R[3].first_prim == 5 && R[3].n_prims == 2 && R[3].movers == 1);
    CHECK(L.facts.n_runs == 4 && L.facts.n_plain_runs == 2 && L.facts.n_ysph_runs == 0);
    CHECK(L.facts.features == F_GBVH && L.facts.bvh_motion);
    const dev_entry* E = arr<dev_entry>(L.mem64, L.at64.entries);
    CHECK(E[4].movers == 1 && E[5].movers == 0 && E[3].bvh_root == 0 && E[2].n_ops == 1 && E[2].first_op == 1);
    const dev_op* O = arr<dev_op>(L.mem64, L.at64.ops);
    CHECK(L.at64.ops.bytes == 2 * sizeof(dev_op) && O[0].type == RTW_OP_FLIP && O[1].type == RTW_OP_ROTATE_Y);
    CHECK(O[1].p[0] == 0.6 && O[1].p[1] == 0.8);

    // movers is OR-ed over the merged entries: the mover in the second of three
    hand g;
    g.sphere(8, 0, 0, 1), g.mover(1, 2, 3, 0.5, 2, 2, 3, 0.0, 1.0), g.sphere(9, 0, 0, 1);
    g.group(0, 1), g.group(1, 1), g.group(2, 1);
    CHECK(g.layout(&L) == RTW_OK);
    R = arr<world_run>(L.mem64, L.at64.runs);
    CHECK(L.s.n_runs == 1 && R[0].entry == WORLD_RUN_PLAIN && R[0].first_prim == 0 && R[0].n_prims == 3);
    CHECK(R[0].movers == 1);
    E = arr<dev_entry>(L.mem64, L.at64.entries);
    CHECK(E[0].movers == 0 && E[1].movers == 1 && E[2].movers == 0);
}

void frames() {
    hand h;
    h.rect(RTW_PRIM_RECT_XZ, 0, 1, 0, 1, 2, 1);
    h.rect(RTW_PRIM_RECT_YZ, 0, 1, 0, 1, 2, 1);
    h.sphere(0, 1, 0, 1);
    const int e = h.group(0, 3);
    h.op(e, RTW_OP_ROTATE_Y, 0.6, 0.8);  // (sin, cos), the outer op
    h.op(e, RTW_OP_FLIP);
    scene_layout L;
    CHECK(h.layout(&L) == RTW_OK);
    CHECK(L.at64.prim_onb.bytes == 3 * 9 * 8 && L.at32.frames.bytes == 3 * 9 * 4);
    const double* F = arr<double>(L.mem64, L.at64.prim_onb);
    const float* F32 = arr<float>(L.mem32, L.at32.frames);
    // +y, the prim's flip, the flip op, rotate_y: +y again.  +x, flipped
    // twice, rotated: (c x + s z, y, -s x + c z) = (0.8, 0, -0.6)
    const d3 want[2] = {d3{0, 1, 0}, d3{0.8, 0, -0.6}};
    for (int p = 0; p < 2; ++p) {
        const onb b = onb_from_w(want[p]);
        const double f[9] = {b.u.x, b.u.y, b.u.z, b.v.x, b.v.y, b.v.z, b.w.x, b.w.y, b.w.z};
        for (int k = 0; k < 9; ++k) CHECK(same(F[9 * p + k], f[k]) && same(F32[9 * p + k], (float)f[k]));
    }
    CHECK(F[6] == 0.0 && F[7] == 1.0 && F[8] == 0.0);  // w of the XZ rect
    for (int k = 18; k < 27; ++k) CHECK(same(F[k], 0.0) && same(F32[k], 0.0f));  // a sphere's frame stays 0
}

void items_and_boxes() {
    {  // world-BVH leaves over plain one-prim entries become ~prim
        hand h;
        h.sphere(0, 1, 0, 1), h.sphere(3, 1, 0, 1), h.sphere(6, 1, 0, 1), h.sphere(7, 1, 0, 1);
        h.group(0, 1), h.group(1, 1);
        h.op(h.group(2, 1), RTW_OP_TRANSLATE, 1, 0, 0);  // not plain: stays an entry
        h.group(3, 1);
        h.items = {1, 0, 2, 3};
        const int l0 = h.leaf(0, 2), l1 = h.leaf(2, 2);
        h.world_root = h.inner(l0, l1);
        scene_layout L;
        CHECK(h.layout(&L) == RTW_OK);
        const int32_t* I = arr<int32_t>(L.mem64, L.at64.items);
        CHECK(L.at64.items.bytes == 16 && I[0] == ~1 && I[1] == ~0 && I[2] == 2 && I[3] == ~3);
        CHECK(L.facts.features == F_WBVH && L.s.world_bvh_root == 0 && L.s.n_nodes == 3);
        // a two-item world leaf is left in index form in the fp32 copy
        const bvh_node32* N = arr<bvh_node32>(L.mem64, L.at64.nodes);
        const bvh_node32* NF = arr<bvh_node32>(L.mem32, L.at32.nodes);
        CHECK(N[1].a == 0 && N[1].b == -2 && NF[1].a == 0 && NF[1].b == -2 && NF[2].a == 2 && NF[2].b == -2);
        CHECK(L.at64.boxes.bytes == 0 && L.at32.boxes.bytes == 0);
    }
    hand h;
    const int b0 = h.box(0, 1, 2, 3, 4, 5), b1 = h.box(10, 11, 12, 13, 14, 15);
    h.items = {RTW_ITEM_BOX | b1, RTW_ITEM_BOX | b0};
    h.group(0, 12, h.leaf(0, 2));
    scene_layout L;
    CHECK(b0 == 0 && b1 == 6 && h.layout(&L) == RTW_OK);
    // records {x0, x1, y0, y1, z0, z1, first rect (int)}, densely, in item order
    CHECK(L.at64.boxes.bytes == 2 * 64 && L.at32.boxes.bytes == 2 * 32);
    const double* B = arr<double>(L.mem64, L.at64.boxes);
    const float* BF = arr<float>(L.mem32, L.at32.boxes);
    for (int k = 0; k < 6; ++k) {
        CHECK(B[k] == 10 + k && B[8 + k] == k && BF[k] == 10 + k && BF[8 + k] == k);
    }
    int32_t first[4];
    std::memcpy(&first[0], B + 6, 4), std::memcpy(&first[1], B + 14, 4);
    std::memcpy(&first[2], BF + 6, 4), std::memcpy(&first[3], BF + 14, 4);
    CHECK(first[0] == 6 && first[1] == 0 && first[2] == 6 && first[3] == 0 && B[7] == 0.0 && BF[15] == 0.0f);
    const int32_t* I = arr<int32_t>(L.mem64, L.at64.items);
    CHECK(I[0] == (RTW_ITEM_BOX | 0) && I[1] == (RTW_ITEM_BOX | 1));
    // the fp32 copy's two-item group leaf holds both items
    const bvh_node32* NF = arr<bvh_node32>(L.mem32, L.at32.nodes);
    CHECK(NF[0].a == (RTW_ITEM_BOX | 0) && NF[0].b == (int32_t)(INT_MIN | RTW_ITEM_BOX | 1));
    CHECK(arr<bvh_node32>(L.mem64, L.at64.nodes)[0].a == 0 && arr<bvh_node32>(L.mem64, L.at64.nodes)[0].b == -2);
    CHECK(L.facts.features == F_GBVH && L.facts.group_depth == 1 && L.facts.stack_need == 3);

    // box_table = false: no table, the items keep RTW_ITEM_BOX | first rect
    CHECK(h.layout(&L, false) == RTW_OK);
    I = arr<int32_t>(L.mem64, L.at64.items);
    CHECK(L.at64.boxes.bytes == 0 && L.at32.boxes.bytes == 0 && I[0] == (RTW_ITEM_BOX | 6) && I[1] == (RTW_ITEM_BOX | 0));
    // one rect of one box off by one ulp: likewise
    h.prims[8].p[1] = std::nextafter(11.0, 12.0);
    CHECK(h.layout(&L) == RTW_OK);
    I = arr<int32_t>(L.mem64, L.at64.items);
    CHECK(L.at64.boxes.bytes == 0 && L.at32.boxes.bytes == 0 && I[0] == (RTW_ITEM_BOX | 6) && I[1] == (RTW_ITEM_BOX | 0));
    NF = arr<bvh_node32>(L.mem32, L.at32.nodes);
    CHECK(NF[0].a == (RTW_ITEM_BOX | 6) && NF[0].b == (int32_t)(INT_MIN | RTW_ITEM_BOX | 0));
}

void nodes() {
    hand h;
    h.sphere(0, 1, 0, 1), h.sphere(3, 1, 0, 1);
    h.group(0, 1), h.group(1, 1);
    h.items = {0, 1};
    const int l = h.leaf(0, 1), r = h.leaf(1, 1);
    h.world_root = h.inner(l, r);
    // the left child's centre is the upper one along z, where they differ most
    const double lo[3] = {0.1, -0.7, 4.0}, hi[3] = {0.7, -0.1, 5.0};
    for (int k = 0; k < 3; ++k) h.nodes[l].bmin[k] = lo[k], h.nodes[l].bmax[k] = hi[k];
    h.nodes[r].bmin[2] = 1.0, h.nodes[r].bmax[2] = 2.0;
    h.nodes[2].bmin[0] = -300.5, h.nodes[2].bmax[2] = 5.0;
    scene_layout L;
    CHECK(h.layout(&L) == RTW_OK);
    const bvh_node32* N = arr<bvh_node32>(L.mem64, L.at64.nodes);
    const bvh_node32* NF = arr<bvh_node32>(L.mem32, L.at32.nodes);
    CHECK(L.at64.nodes.bytes == 3 * 32 && L.at32.nodes.bytes == 3 * 32 && L.s.world_bvh_root == 0);
    // BFS: the root first, then its children
    CHECK(N[0].a == 1 && N[0].b == (2 | (2 << 28) | (4 << 28)));
    CHECK(same(N[0].lo[0], -300.5f) && same(N[0].hi[2], 5.0f));
    // bounds rounded outward, on both sides
    CHECK(same(N[1].lo[0], 0x1.999998p-4f) && same(N[1].hi[0], 0x1.666668p-1f));
    CHECK(same(N[1].lo[1], -0x1.666668p-1f) && same(N[1].hi[1], -0x1.999998p-4f));
    CHECK(same(N[1].lo[2], 4.0f) && same(N[1].hi[2], 5.0f));
    CHECK(N[1].a == 0 && N[1].b == -1 && N[2].a == 1 && N[2].b == -1);
    // fp32 copy: a one-item leaf holds its item (~prim here)
    CHECK(NF[1].a == ~0 && NF[1].b == -1 && NF[2].a == ~1 && NF[2].b == -1 && NF[0].a == 1 && NF[0].b == N[0].b);
    CHECK(same(NF[1].lo[0], N[1].lo[0]) && same(NF[1].hi[1], N[1].hi[1]));
    CHECK(L.s.bvh_bound == 300.5 && L.facts.stack_need == 4 && L.facts.group_depth == 0);
}

hand bfs_scene() {
    hand h;
    for (int k = 0; k < 4; ++k) h.sphere(3 * k, 1, 0, 1);
    h.items = {0, 1, 2, 3, 0, 1, 3};
    h.leaf(0, 1);                   // 0: group A's left leaf
    h.leaf(1, 1);                   // 1: group A's right leaf
    h.leaf(6, 1);                   // 2: unreachable
    h.leaf(2, 2);                   // 3: group B's root
    h.leaf(4, 1);                   // 4: world leaf (entry 0)
    h.inner(0, 1);                  // 5: group A's root
    h.world_root = h.inner(4, 7);   // 6: the world root
    h.leaf(5, 1);                   // 7: world leaf (entry 1)
    h.nodes[4].bmin[1] = 7.0, h.nodes[4].bmax[1] = 8.0;  // world root: split along y, left upper
    h.nodes[1].bmin[0] = 2.0, h.nodes[1].bmax[0] = 3.0;  // group A: along x, right upper
    h.group(0, 2, 5), h.group(2, 2, 3);
    return h;
}

void bfs() {
    const hand h = bfs_scene();
    scene_layout L;
    CHECK(h.layout(&L) == RTW_OK);
    // 6 -> 0, 5 -> 1, 3 -> 2; then level by level: 4 -> 3, 7 -> 4, 0 -> 5, 1 -> 6; 2 keeps a slot: 7
    const bvh_node32* N = arr<bvh_node32>(L.mem64, L.at64.nodes);
    const bvh_node32* NF = arr<bvh_node32>(L.mem32, L.at32.nodes);
    const dev_entry* E = arr<dev_entry>(L.mem64, L.at64.entries);
    CHECK(L.s.world_bvh_root == 0 && L.s.n_nodes == 8 && L.at64.nodes.bytes == 8 * 32);
    CHECK(E[0].bvh_root == 1 && E[1].bvh_root == 2);
    CHECK(N[0].a == 3 && N[0].b == (4 | (1 << 28) | (4 << 28)));
    CHECK(N[1].a == 5 && N[1].b == (6 | (0 << 28)));
    CHECK(N[2].a == 2 && N[2].b == -2 && N[3].a == 4 && N[3].b == -1 && N[4].a == 5 && N[4].b == -1);
    CHECK(N[5].a == 0 && N[5].b == -1 && N[6].a == 1 && N[6].b == -1 && N[7].a == 6 && N[7].b == -1);
    CHECK(same(N[3].lo[1], 7.0f) && same(N[6].hi[0], 3.0f));
    // the fp32 copy, inline: entries in world leaves, prims in group leaves
    CHECK(NF[0].a == 3 && NF[0].b == N[0].b && NF[3].a == 0 && NF[4].a == 1 && NF[5].a == 0 && NF[6].a == 1);
    CHECK(NF[2].a == 2 && NF[2].b == (int32_t)(INT_MIN | 3) && NF[7].a == 3 && NF[7].b == -1);
    const rtwf::ent32* EF = arr<rtwf::ent32>(L.mem32, L.at32.entries);
    CHECK(EF[0].bvh_root == 1 && EF[1].bvh_root == 2);
    CHECK(L.facts.features == (F_WBVH | F_GBVH) && L.facts.n_nodes == 8);
    CHECK(L.facts.group_depth == 2 && L.facts.stack_need == 2 + 2 + 2);
    const int32_t* I = arr<int32_t>(L.mem64, L.at64.items);
    CHECK(I[4] == 0 && I[5] == 1);  // entries with a BVH stay entries
}

void bad_bounds() {
    const double bad[2] = {INFINITY, 0x1p91};
    for (double v : bad) {
        hand h = bfs_scene();
        h.nodes[3].bmax[2] = v;
        scene_layout L;
        CHECK(h.layout(&L) == RTW_OK);
        CHECK(L.s.world_bvh_root == -1 && L.s.n_nodes == 0 && L.facts.n_nodes == 0);
        CHECK((L.facts.features & (F_WBVH | F_GBVH)) == 0);
        const rtwf::ent32* EF = arr<rtwf::ent32>(L.mem32, L.at32.entries);
        CHECK(EF[0].bvh_root == -1 && EF[1].bvh_root == -1);
    }
    hand h = bfs_scene();
    h.nodes[3].bmax[2] = 0x1p90;  // the largest bound a BVH may have
    scene_layout L;
    CHECK(h.layout(&L) == RTW_OK && L.s.n_nodes == 8 && L.s.bvh_bound == 0x1p90);
}

// A world BVH that is one chain: `depth` levels, a leaf hanging off every
// inner node.
hand chain(int depth) {
    hand h;
    for (int k = 0; k < depth; ++k) {
        h.sphere(3 * k, 1, 0, 1);
        h.group(k, 1);
        h.items.push_back(k);
    }
    int below = h.leaf(depth - 1, 1);
    for (int k = depth - 2; k >= 0; --k) below = h.inner(h.leaf(k, 1), below);
    h.world_root = below;
    return h;
}

void depth() {
    scene_layout L;
    CHECK(kStack == 48);
    CHECK(chain(kStack - 2).layout(&L) == RTW_OK);
    CHECK(L.facts.stack_need == kStack && L.facts.group_depth == 0 && L.s.n_nodes == 2 * (kStack - 2) - 1);
    CHECK(chain(kStack - 1).layout(&L) == RTW_ERR_UNSUPPORTED);
    CHECK(std::string(rtw_last_error()) == "BVH too deep for the traversal stack (49 > 48 entries)");
}

void media_walk() {
    hand h;
    h.sphere(0, 1, 0, 1), h.sphere(3, 1, 0, 1), h.sphere(6, 1, 0, 1);
    h.materials.resize(1);
    std::memset(h.materials.data(), 0, sizeof(rtw_material));
    h.materials[0].type = RTW_MAT_ISOTROPIC;
    h.group(0, 1), h.group(1, 1), h.group(2, 1);
    h.entries[1].kind = RTW_ENTRY_MEDIUM, h.entries[1].density = 0.5, h.entries[1].phase_material = 0;
    scene_layout L;
    // without a program: every entry, then the media again
    CHECK(h.layout(&L) == RTW_OK);
    const int32_t* M = arr<int32_t>(L.mem64, L.at64.media);
    CHECK(L.s.n_media == 4 && L.at64.media.bytes == 16 && M[0] == 0 && M[1] == 1 && M[2] == 2 && M[3] == 1);
    CHECK(L.s.has_media == 1 && L.facts.features == F_MEDIA && L.facts.shade_mask == SF_ISO);
    CHECK(arr<dev_entry>(L.mem64, L.at64.entries)[1].neg_inv_density == -2.0);
    CHECK(arr<dev_entry>(L.mem64, L.at64.entries)[0].neg_inv_density == 0.0);
    CHECK(same(arr<rtwf::ent32>(L.mem32, L.at32.entries)[1].neg_inv_density, -2.0f));
    // with a program: replays of non-media entries dropped, media replays kept
    h.visits = {1, 0, RTW_VISIT_REPLAY | 1, RTW_VISIT_REPLAY | 0, 2, RTW_VISIT_REPLAY | 2};
    CHECK(h.layout(&L) == RTW_OK);
    M = arr<int32_t>(L.mem64, L.at64.media);
    CHECK(L.s.n_media == 4 && M[0] == 1 && M[1] == 0 && M[2] == 1 && M[3] == 2);
    // no medium: no walk
    h.entries[1].kind = RTW_ENTRY_GROUP;
    CHECK(h.layout(&L) == RTW_OK && L.s.n_media == 0 && L.at64.media.bytes == 0 && L.s.has_media == 0);
    CHECK(L.facts.features == 0);
}

void masks() {
    hand h;
    h.sphere(0, 1, 0, 1), h.rect(RTW_PRIM_RECT_XZ, 0, 1, 0, 1, 2), h.sphere(6, 1, 0, 1);
    h.op(h.group(0, 2), RTW_OP_TRANSLATE, 1, 2, 3);
    h.group(2, 1);
    const int mat[3] = {RTW_MAT_LAMBERTIAN, RTW_MAT_METAL, RTW_MAT_DIELECTRIC};
    const int tex[2] = {RTW_TEX_CONSTANT, RTW_TEX_CHECKER};
    for (int t : mat) {
        rtw_material m;
        std::memset(&m, 0, sizeof m);
        m.type = t, m.ref_idx = 1.5;
        h.materials.push_back(m);
    }
    for (int t : tex) {
        rtw_texture x;
        std::memset(&x, 0, sizeof x);
        x.type = t;
        h.textures.push_back(x);
    }
    h.lights = {{RTW_LIGHT_XZ_RECT, 1}, {RTW_LIGHT_SPHERE, 2}, {RTW_LIGHT_SPHERE, 0}};
    scene_layout L;
    CHECK(h.layout(&L) == RTW_OK);
    CHECK(L.facts.shade_mask == (SF_METAL | SF_DIEL | SF_CHECKER) && L.facts.lights && L.s.n_lights == 3);
    CHECK(same(L.s.light_weight, 1.0 / 3.0) && same(L.s.f_light_weight, (float)(1.0 / 3.0)));
    // material.h:158 1 / ref_idx, :46-47 r0 = ((1 - ri) / (1 + ri))^2
    const double* A = arr<double>(L.mem64, L.at64.mat_aux);
    CHECK(same(A[4], 1.0 / 1.5) && same(A[5], (-0.5 / 2.5) * (-0.5 / 2.5)));
    // the shading prefix: prims, entries, materials, textures, lights,
    // (no Perlin tables, no media), frames, mat_aux, ops
    const size_t prefix = al(3 * 96) + al(2 * 48) + al(3 * 48) + al(2 * 48) + al(3 * 8) + al(3 * 72) + al(3 * 16) + al(32);
    CHECK(L.facts.shade_bytes == prefix && L.at64.nodes.off == prefix && L.at64.nodes.bytes == 0);
    CHECK(L.at64.ranvec.bytes == 0 && L.at64.perm.bytes == 0 && L.at64.items.off == prefix);
    // fp32: prims, entries, ops, materials, textures, (ranvec), frames, lights, (perm)
    const size_t end32 = al(3 * 64) + al(2 * 48) + al(16) + al(3 * 40) + al(2 * 32) + al(3 * 36) + al(3 * 8);
    CHECK(L.facts.f32_bytes == end32 && L.at32.perm.off == end32 && L.at32.perm.bytes == 0);
    CHECK(L.mem32.size() == end32 && L.mem64.size() % 256 == 0);
    CHECK(L.facts.black);  // (black background, colour rendering)

    // the Book-2 set with Perlin tables and an image
    h.materials[0].type = RTW_MAT_ISOTROPIC;
    h.textures[1].type = RTW_TEX_NOISE;
    h.textures[0].type = RTW_TEX_IMAGE;
    h.ranvec.assign(768, 0.25), h.perm.assign(768, 7);
    rtw_scene_desc d = h.desc();
    const uint8_t texels[5] = {1, 2, 3, 4, 5};
    d.image_texels = texels, d.image_bytes = 5;
    d.background = RTW_BG_GRADIENT;
    CHECK(rtw_layout_scene(&d, true, &L) == RTW_OK);
    CHECK(L.facts.shade_mask == (SF_ISO | SF_METAL | SF_DIEL | SF_NOISE | SF_IMAGE) && !L.facts.black);
    CHECK(L.facts.shade_bytes == prefix + al(768 * 8) + al(768 * 4) && L.facts.shade_bytes == L.at64.nodes.off);
    CHECK(L.facts.f32_bytes == end32 + al(768 * 4) + 768 * 4 && L.at32.perm.off + L.at32.perm.bytes == L.facts.f32_bytes);
    CHECK(L.at64.texels.bytes == 5 && std::memcmp(L.mem64.data() + L.at64.texels.off, texels, 5) == 0);
    CHECK(L.mem64.size() == L.at64.texels.off + 256);
    CHECK(arr<int32_t>(L.mem32, L.at32.perm)[767] == 7 && same(arr<float>(L.mem32, L.at32.ranvec)[767], 0.25f));
    // selection reads the facts as they are
    const select_in s = rtw_layout_select_in(L.facts, true);
    CHECK(s.features == L.facts.features && s.shade_mask == L.facts.shade_mask && s.shade_bytes == L.facts.shade_bytes);
    CHECK(s.f32_bytes == L.facts.f32_bytes && s.lights && !s.black && s.pin && s.static_scene && !s.ysph && !s.strict);
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "scenes" && argc == 3) return dump_scenes(argv[2]);
    if (mode != "cases") return 2;
    ysphere_runs();
    movers();
    runs();
    frames();
    items_and_boxes();
    nodes();
    bfs();
    bad_bounds();
    depth();
    media_walk();
    masks();
    if (g_failed) {
        std::printf("%d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    std::printf("OK (%d checks)\n", g_checks);
    return 0;
}
