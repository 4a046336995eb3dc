// select_check.cpp — walks kernel selection (rtw_select.h) over the grids of
// tests/golden/kernel_selection.json and prints one kernel name per row, in
// that file's order; "# <precision> <build> <RTW_SORT | RTW_FAST_SORT>" starts
// each block.  Exits 1 when a choice has no entry in its family's list (the
// launch tables of rtw_kernels.hip are built from those lists), or when a
// split choice resolves to other rows than the launch switches once named.
#include <cstdio>
#include "rtw_select.h"

using namespace rtwd;

static int g_unlisted = 0;

// The split pair as the launch switches named it before the launch tables
// held it: k_shade's `case M * 2 + LDS` labels and k_intersect's `case F`
// labels, with what their `default:` rows launched.
struct shade_label {
    int m;
    bool lds;
};
static const shade_label kShadeLabels[] = {{SF_DIEL, true},  {SF_DIEL, false},  {SF_METAL | SF_DIEL, true},
                                           {SF_METAL | SF_DIEL, false}, {SF_NOISE, true}, {SF_NOISE, false},
                                           {SF_ALL, true},   {SF_IMG_ALL, false}};
static const shade_label kShadeDefault = {SF_ALL, false};  // ... with 0 bytes of LDS
static const int kIntersectLabels[] = {0, F_MEDIA, F_WBVH, F_GBVH, F_MEDIA | F_GBVH, F_WBVH | F_GBVH};
static const int kIntersectDefault = F_MEDIA | F_GBVH;

// the rows of a split choice: in the lists, and the switches' instantiations
static int split_at(const kernel_choice& c) {
    const split_rows r = split_resolve(c.id);
    if (index_of(kIntersectList, r.intersect) < 0 || index_of(kShadeList, r.shade) < 0) return -1;
    shade_label s = kShadeDefault;
    for (const shade_label& l : kShadeLabels)
        if (l.m * 2 + (l.lds ? 1 : 0) == c.id.m * 2 + (c.id.l ? 1 : 0)) s = l;
    int f = kIntersectDefault;
    for (int l : kIntersectLabels)
        if (l == c.id.f) f = l;
    // (LDS bytes: the switch passed the shading data's when the label's LDS
    // was set, 0 in the default row -- the resolved row's l says the same)
    const bool same = r.shade.f == -1 && r.shade.m == s.m && r.shade.l == s.lds && r.intersect.f == f &&
                      r.intersect.m == -1 && !r.intersect.l;
    if (!same)
        std::fprintf(stderr, "split {%d, %d, %d}: rows k_intersect<%d> k_shade<%d, %d>, the switches' k_intersect<%d> "
                             "k_shade<%d, %d>\n", c.id.f, c.id.m, c.id.l, r.intersect.f, r.shade.m, r.shade.l, f, s.m, s.lds);
    return same ? 0 : -1;
}

static void print(const kernel_choice& c) {
    int at = 0;
    switch (c.form) {
    case kform::persist_sort:
    case kform::persist:
    case kform::persist_lst: at = index_of(kPersistList, c.id); break;
    case kform::segment: at = index_of(kSegmentList, c.id); break;
    case kform::fast: at = index_of(kFastList, c.id); break;
    case kform::fast_sort: at = index_of(kFastSortList, c.id); break;
    case kform::split: at = split_at(c); break;
    }
    if (at < 0) {
        std::fprintf(stderr, "no such instantiation: %s\n", c.name.c_str());
        ++g_unlisted;
    }
    std::puts(c.name.c_str());
}

int main() {
    const int masks[] = {0, SF_CHECKER, SF_METAL, SF_DIEL, SF_METAL | SF_DIEL, SF_NOISE, SF_NOCHECKER, SF_ALL,
                         SF_IMAGE | SF_DIEL};
    const uint32_t bytes[] = {1024, 41 * 1024};
    const int stack_nodes[3][2] = {{kLdsStack, 1000}, {kLdsStack + 1, 1000}, {kLdsStack, 65536}};
    const char* sort_name[] = {"unset", "0", "1"};
    for (int strict = 0; strict < 2; ++strict)
        for (int sort = -1; sort < 2; ++sort) {
            std::printf("# fp64 %s %s\n", strict ? "strict" : "default", sort_name[sort + 1]);
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
                                        print(select_fp64(s));
                                    }
        }
    const int fast_masks[] = {0, SF_NOISE, SF_IMAGE, SF_IMAGE | SF_NOISE};
    const int nodes[] = {1000, 65536};
    for (int strict = 0; strict < 2; ++strict)
        for (int fast_sort = 1; fast_sort >= 0; --fast_sort) {
            std::printf("# fp32 %s %s\n", strict ? "strict" : "default", fast_sort ? "unset" : "0");
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
                                    s.strict = strict;
                                    print(select_fp32(s));
                                }
        }
    // the split pair's lists name exactly the switches' instantiations
    size_t named = index_of(kShadeList, inst{-1, kShadeDefault.m, kShadeDefault.lds}) >= 0 ? 1 : 0;
    for (const shade_label& l : kShadeLabels) named += index_of(kShadeList, inst{-1, l.m, l.lds}) >= 0 ? 1 : 0;
    size_t named_f = 0;
    for (int f : kIntersectLabels) named_f += index_of(kIntersectList, inst{f, -1, false}) >= 0 ? 1 : 0;
    if (named != kShadeList.size() || named != 9 || named_f != kIntersectList.size() || named_f != 6 ||
        index_of(kIntersectList, inst{kIntersectDefault, -1, false}) < 0) {
        std::fprintf(stderr, "kShadeList / kIntersectList differ from the launch switches' labels\n");
        return 1;
    }
    return g_unlisted ? 1 : 0;
}
