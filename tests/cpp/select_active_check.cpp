// select_active_check.cpp — kernel selection of an active render (rtw_select.h
// select_active, rtw_adaptive.h) over select_check.cpp's grids: every
// (scene facts, precision, environment) combination with `active` set maps to
// a row of the active lists or, fp64, to a wavefront form whose rows are
// listed -- never to nothing -- and the same facts with `active` unset give
// what select_fp64 / select_fp32 give without the field.  Prints the number of
// choices per kind and the kernels of the built-in scenes' facts; exits 1 on
// the first kind of failure it finds.
#include <cstdio>
#include <map>
#include <string>
#include "rtw_select.h"

using namespace rtwd;

static int g_bad = 0;
static std::map<std::string, long> g_kinds;

#define FAIL(...) (std::fprintf(stderr, __VA_ARGS__), std::fputc('\n', stderr), ++g_bad)

static bool same(const kernel_choice& a, const kernel_choice& b) {
    return a.form == b.form && a.id == b.id && a.name == b.name && a.active == b.active;
}

static void check_fp64(select_in s) {
    s.active = false;
    const kernel_choice whole = select_fp64(s);
    if (whole.active) FAIL("fp64: a whole-image choice is marked active: %s", whole.name.c_str());
    s.active = true;
    const kernel_choice c = select_fp64(s);
    if (!same(c, select_active(s, false))) FAIL("fp64: select_fp64 with active set is not select_active");
    if (!c.active) FAIL("fp64: an active choice is not marked: %s", c.name.c_str());
    if (c.persistent()) {
        // a row of the active list, the whole-image kernel with the bit, in its form
        if (index_of(kPersistActiveList, active_inst{c.id, c.form}) < 0) FAIL("no such active row: %s", c.name.c_str());
        if (!(c.id.f & F_ACTIVE) || (c.id.f & ~F_ACTIVE) != whole.id.f || c.id.m != whole.id.m || c.id.l != whole.id.l ||
            c.form != whole.form)
            FAIL("active %s is not the whole-image %s with the bit", c.name.c_str(), whole.name.c_str());
        if (s.strict) FAIL("strict: a persistent active choice %s", c.name.c_str());
        ++g_kinds["fp64 persistent"];
        return;
    }
    // the wavefront route: what RTW_MODE=wavefront selects, refilled by k_regen_active
    select_in w = s;
    w.active = false, w.env.wavefront = true;
    const kernel_choice want = select_fp64(w);
    if (c.form != want.form || !(c.id == want.id) || c.name != "k_regen_active + " + want.name)
        FAIL("wavefront route %s differs from RTW_MODE=wavefront's %s", c.name.c_str(), want.name.c_str());
    if (c.id.f & F_ACTIVE) FAIL("a wavefront kernel with the bit: %s", c.name.c_str());
    if (c.form == kform::segment) {
        if (index_of(kSegmentList, c.id) < 0) FAIL("no such instantiation: %s", c.name.c_str());
        ++g_kinds["fp64 k_regen_active + k_segment"];
    } else {
        const split_rows r = split_resolve(c.id);
        if (index_of(kIntersectList, r.intersect) < 0 || index_of(kShadeList, r.shade) < 0)
            FAIL("split rows of %s are not listed", c.name.c_str());
        ++g_kinds["fp64 k_regen_active + split pair"];
    }
}

static void check_fp32(select_in s) {
    s.active = false;
    const kernel_choice whole = select_fp32(s);
    s.active = true;
    if (!active_fp32_ok(s)) {  // refused before selection (image textures)
        if (!(s.shade_mask & SF_IMAGE)) FAIL("fp32: refused without image textures");
        ++g_kinds["fp32 refused (image textures)"];
        return;
    }
    const kernel_choice c = select_fp32(s);
    if (!same(c, select_active(s, true))) FAIL("fp32: select_fp32 with active set is not select_active");
    if (!c.active || !(c.id.f & F_ACTIVE)) FAIL("fp32: an active choice without the bit: %s", c.name.c_str());
    const int at = c.form == kform::fast        ? index_of(kFastActiveList, active_inst{c.id, c.form})
                   : c.form == kform::fast_sort ? index_of(kFastSortActiveList, active_inst{c.id, c.form}) : -1;
    if (at < 0) FAIL("no such active row: %s", c.name.c_str());
    const bool exact = (c.id.f & ~F_ACTIVE) == whole.id.f && c.id.l == whole.id.l && c.form == whole.form;
    if (!exact) {
        // a general row: k_fast of the scene's walk (world BVH, media, list), group BVHs
        // tested per entry, every texture, private stacks
        const int f = s.features & (F_MEDIA | F_WBVH | F_GBVH);
        const int walk = (f & F_MEDIA) ? F_MEDIA : (f & F_WBVH) ? F_WBVH : 0;
        if (c.form != kform::fast || c.id.l || c.id.f != (walk | F_GBVH | F_ACTIVE))
            FAIL("fp32: %s is neither the whole-image %s with the bit nor its walk's general row", c.name.c_str(),
                 whole.name.c_str());
    }
    ++g_kinds[exact ? "fp32 the whole-image kernel with the bit" : "fp32 general k_fast of the walk"];
}

int main() {
    const int masks[] = {0, SF_CHECKER, SF_METAL, SF_DIEL, SF_METAL | SF_DIEL, SF_NOISE, SF_NOCHECKER, SF_ALL,
                         SF_IMAGE | SF_DIEL};
    const uint32_t bytes[] = {1024, 41 * 1024};
    const int stack_nodes[3][2] = {{kLdsStack, 1000}, {kLdsStack + 1, 1000}, {kLdsStack, 65536}};
    for (int strict = 0; strict < 2; ++strict)
        for (int sort = -1; sort < 2; ++sort)
            for (int f = 0; f < 8; ++f)
                for (int mask : masks)
                    for (uint32_t b : bytes)
                        for (auto& sn : stack_nodes)
                            for (int bits = 0; bits < 32; ++bits)
                                for (int wavefront = 0; wavefront < 2; ++wavefront)
                                    for (int split = 0; split < 2; ++split) {
                                        select_in s;
                                        s.features = f, s.shade_mask = mask, s.shade_bytes = b;
                                        s.stack_need = sn[0], s.n_nodes = sn[1];
                                        s.ysph = bits & 1, s.static_scene = bits & 2, s.lights = bits & 4;
                                        s.black = bits & 8, s.pin = bits & 16;
                                        s.env.wavefront = wavefront, s.env.split = split, s.env.sort = sort;
                                        s.strict = strict;
                                        check_fp64(s);
                                    }
    const int fast_masks[] = {0, SF_NOISE, SF_IMAGE, SF_IMAGE | SF_NOISE};
    const int nodes[] = {1000, 65536};
    for (int fast_sort = 1; fast_sort >= 0; --fast_sort)
        for (int f = 0; f < 8; ++f)
            for (int mask : fast_masks)
                for (uint32_t b : bytes)
                    for (int ds = 0; ds < 2; ++ds)
                        for (int dg = 0; dg < 2; ++dg)
                            for (int n : nodes) {
                                select_in s;
                                s.features = f, s.shade_mask = mask, s.f32_bytes = b;
                                s.stack_need = rtwf::fast_stack(f) + ds, s.group_depth = rtwf::fast_stack(f) + dg;
                                s.n_nodes = n;
                                s.env.fast_sort = fast_sort != 0;
                                check_fp32(s);
                            }
    // every row of the active lists carries the bit and is some whole-image row with it
    for (const active_inst& a : kPersistActiveList)
        if (!(a.id.f & F_ACTIVE) || index_of(kPersistList, inst{a.id.f & ~F_ACTIVE, a.id.m, a.id.l}) < 0)
            FAIL("kPersistActiveList: <%d, %d, %d> is no kPersistList row with the bit", a.id.f, a.id.m, a.id.l);
    for (const active_inst& a : kFastActiveList)
        if (!(a.id.f & F_ACTIVE) || index_of(kFastList, inst{a.id.f & ~F_ACTIVE, -1, a.id.l}) < 0)
            FAIL("kFastActiveList: <%d, %d> is no kFastList row with the bit", a.id.f, a.id.l);
    for (const active_inst& a : kFastSortActiveList)
        if (!(a.id.f & F_ACTIVE) || index_of(kFastSortList, inst{a.id.f & ~F_ACTIVE, -1, a.id.l}) < 0)
            FAIL("kFastSortActiveList: <%d, %d> is no kFastSortList row with the bit", a.id.f, a.id.l);
    // the built-in scenes' facts (tests/golden/scene_query_gfx950.json names their whole-image kernels)
    struct {
        const char* name;
        select_in s;
    } scenes[4];
    scenes[0].name = "cornell_box";
    scenes[0].s.shade_mask = SF_DIEL, scenes[0].s.shade_bytes = scenes[0].s.f32_bytes = 4608;
    scenes[0].s.static_scene = scenes[0].s.lights = scenes[0].s.black = true;
    scenes[1].name = "random_balls";
    scenes[1].s.shade_mask = SF_METAL | SF_DIEL, scenes[1].s.shade_bytes = scenes[1].s.f32_bytes = 64 * 1024;
    scenes[1].s.ysph = true;
    scenes[2].name = "random_balls/bvh";
    scenes[2].s = scenes[1].s;
    scenes[2].s.features = F_WBVH, scenes[2].s.stack_need = 12, scenes[2].s.n_nodes = 969;
    scenes[3].name = "book2_final/bvh";
    scenes[3].s.features = F_MEDIA | F_GBVH, scenes[3].s.shade_mask = SF_NOCHECKER;
    scenes[3].s.shade_bytes = scenes[3].s.f32_bytes = 64 * 1024;
    scenes[3].s.stack_need = 12, scenes[3].s.group_depth = 12, scenes[3].s.n_nodes = 1668;
    scenes[3].s.lights = scenes[3].s.black = scenes[3].s.pin = true;
    for (auto& x : scenes) {
        x.s.active = true;
        std::printf("scene %s: %s | %s\n", x.name, select_fp64(x.s).name.c_str(), select_fp32(x.s).name.c_str());
    }
    for (auto& k : g_kinds) std::printf("%s: %ld\n", k.first.c_str(), k.second);
    if (g_bad) return 1;
    std::puts("OK");
    return 0;
}
