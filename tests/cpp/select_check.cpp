// select_check.cpp — walks kernel selection (rtw_select.h) over the grids of
// tests/golden/kernel_selection.json and prints one kernel name per row, in
// that file's order; "# <precision> <build> <RTW_SORT | RTW_FAST_SORT>" starts
// each block.  Exits 1 when a choice has no entry in its family's list (the
// launch tables of rtw_kernels.hip are built from those lists).
#include <cstdio>
#include "rtw_select.h"

using namespace rtwd;

static int g_unlisted = 0;

static void print(const kernel_choice& c) {
    int at = 0;
    switch (c.form) {
    case kform::persist_sort:
    case kform::persist:
    case kform::persist_lst: at = index_of(kPersistList, c.id); break;
    case kform::segment: at = index_of(kSegmentList, c.id); break;
    case kform::fast: at = index_of(kFastList, c.id); break;
    case kform::fast_sort: at = index_of(kFastSortList, c.id); break;
    case kform::split: break;  // k_intersect / k_shade: switches with default rows
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
    return g_unlisted ? 1 : 0;
}
