// scene_layout.cpp — rtw_layout_scene: an rtw_scene_desc turned into what the
// kernels read (scene_layout.h).  Host arithmetic only; the values the
// kernels would otherwise compute per test are formed here once with the
// device's expressions (rtw_layout.h), so this file is compiled with
// -ffp-contract=off like the kernels.
#include "scene_layout.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include "rtw_host_util.h"
#include "rtw_layout.h"

using namespace rtwd;
using namespace rtwf;

namespace {

// Everything between the desc and the blobs.
struct work {
    const rtw_scene_desc* d = nullptr;
    std::vector<int32_t> media;  // the media walk
    bool has_media = false;
    std::vector<double> frames, mat_aux;
    std::vector<rtw_prim> prims;  // the device copy of the prims
    bool mv_common = false;
    double mv_t0 = 0.0, mv_den = 1.0;
    std::vector<world_run> runs;
    std::vector<int32_t> entry_movers;
    std::vector<float> ysph;
    float ysb[5] = {0, 0, 0, 0, 0};  // |cx|, |cy|, |dy|, |cz|, r^2 maxima
    std::vector<int32_t> items;
    std::vector<char> world_node;  // (the fp32 nodes' inline world leaves)
    std::vector<int> box_firsts;   // box record -> first rect
    std::vector<double> boxes64;
    std::vector<rtw_bvh_node> nodes;
    std::vector<bvh_node32> nodes32, nodes32f;
    double bvh_bound = 0.0;
    bool bvh_ok = false;
    std::vector<rtw_entry> entries;  // with BFS-renumbered roots
    int world_root = -1;
    std::vector<dev_entry> dev_entries;
    std::vector<dev_op> dev_ops;
};

// The blobs' packer: appends a 256-byte aligned sub-array (zero padded).
layout_span put(std::vector<char>& mem, const void* src, size_t bytes) {
    const layout_span at{mem.size(), bytes};
    mem.resize(at.off + ((bytes + 255) & ~size_t(255)), 0);
    if (bytes && src) std::memcpy(mem.data() + at.off, src, bytes);
    return at;
}
template <class T>
layout_span put(std::vector<char>& mem, const std::vector<T>& v) {
    return put(mem, v.data(), sizeof(T) * v.size());
}

// The media walk (scene::media, world_closest with F_MEDIA): the visit
// program (rtw_scene_desc::visits) without its deterministic replays --
// a second walk over an object with no random draws re-accepts only an
// exact tie -- or, without a program, the world's two walks the same way:
// every entry, then the media again.
void media_walk(work& w) {
    const rtw_scene_desc* d = w.d;
    for (int e = 0; e < d->n_entries; ++e) w.has_media |= d->entries[e].kind == RTW_ENTRY_MEDIUM;
    if (!w.has_media) return;
    if (d->n_visits > 0) {
        for (int k = 0; k < d->n_visits; ++k) {
            const int e = d->visits[k] & RTW_VISIT_ENTRY;
            if (!(d->visits[k] & RTW_VISIT_REPLAY) || d->entries[e].kind == RTW_ENTRY_MEDIUM) w.media.push_back(e);
        }
    } else {
        for (int e = 0; e < d->n_entries; ++e) w.media.push_back(e);
        for (int e = 0; e < d->n_entries; ++e)
            if (d->entries[e].kind == RTW_ENTRY_MEDIUM) w.media.push_back(e);
    }
}

// World-space onb of every rect primitive's normal: rect_normal, the
// prim's own flip, then its entry's ops outward -- hit_record's normal
// path (rtw_device.h) -- and onb_from_w, all with the device's expressions.
// And per material: 1/ref_idx and schlick's r0^2 (material.h:158, :46-47).
void frames_and_materials(work& w) {
    const rtw_scene_desc* d = w.d;
    w.frames.assign((size_t)d->n_prims * 9, 0.0);
    for (int pi = 0; pi < d->n_prims; ++pi) {
        const rtw_prim& q = d->prims[pi];
        if (q.type < RTW_PRIM_RECT_XY || q.entry < 0) continue;
        d3 n = rect_normal(q.type);
        if (q.flip & 1) n = -n;
        const rtw_entry& e = d->entries[q.entry];
        for (int k = RTW_MAX_OPS - 1; k >= 0; --k) {
            if (k >= e.n_ops) continue;
            if (e.op[k] == RTW_OP_ROTATE_Y) {
                const double s = e.op_param[k][0], c = e.op_param[k][1];
                const d3 n0 = n;
                n.x = c * n0.x + s * n0.z;
                n.z = -s * n0.x + c * n0.z;
            } else if (e.op[k] == RTW_OP_FLIP) {
                n = -n;
            }
        }
        const onb b = onb_from_w(n);
        double* f = w.frames.data() + 9 * (size_t)pi;
        f[0] = b.u.x, f[1] = b.u.y, f[2] = b.u.z;
        f[3] = b.v.x, f[4] = b.v.y, f[5] = b.v.z;
        f[6] = b.w.x, f[7] = b.w.y, f[8] = b.w.z;
    }
    w.mat_aux.assign((size_t)d->n_materials * 2, 0.0);
    for (int k = 0; k < d->n_materials; ++k) {
        const double ri = d->materials[k].ref_idx;
        double r0 = (1 - ri) / (1 + ri);
        r0 = r0 * r0;
        w.mat_aux[2 * k] = 1.0 / ri;
        w.mat_aux[2 * k + 1] = r0;
    }
}

// Device copy of the prims: sphere records rewritten as rtw_layout.h
// (DP_MOVING_COMMON) describes -- radius^2, center1 - center0, time1 -
// time0 precomputed with the reference's expressions -- and the moving
// spheres sharing the first mover's interval tagged so traversal computes
// their time fraction once per ray.
void prims_and_movers(work& w) {
    w.prims.assign(w.d->prims, w.d->prims + w.d->n_prims);
    for (rtw_prim& q : w.prims) {
        if (!is_sphere(q.type)) continue;
        q.p[9] = q.p[3] * q.p[3];
        if (q.type != RTW_PRIM_MOVING_SPHERE) continue;
        for (int k = 0; k < 3; ++k) q.p[4 + k] = q.p[4 + k] - q.p[k];
        q.p[8] = q.p[8] - q.p[7];
        // the shared fraction must stay finite: (time - t0) is at most ~2^129
        // in magnitude (light pdf rays carry time FLT_MAX)
        const bool finite_frac = std::isfinite(q.p[7]) && std::isfinite(q.p[8]) && std::fabs(q.p[8]) >= 1e-200;
        if (!finite_frac) continue;
        if (!w.mv_common) {
            w.mv_common = true;
            w.mv_t0 = q.p[7];
            w.mv_den = q.p[8];
        }
        if (std::memcmp(&q.p[7], &w.mv_t0, 8) != 0 || std::memcmp(&q.p[8], &w.mv_den, 8) != 0) continue;
        // y-only mover: x and z stay center0's exactly when dc is +-0 and
        // center0's component is nonzero (x + +-0 == x for x != 0)
        const bool y_only = q.p[4] == 0.0 && q.p[6] == 0.0 && q.p[0] != 0.0 && q.p[2] != 0.0;
        q.type = y_only ? DP_MOVING_COMMON_Y : DP_MOVING_COMMON;
    }
}

// World list runs: consecutive plain entries (one group, no BVH, no op
// that moves the ray -- flip_normals only turns the normal, which
// hit_record applies from the prim's entry) scan their contiguous prims
// as one run.  (Cornell: the flipped walls join the plain ones.)
bool ray_plain(const rtw_entry& E) {
    if (E.kind != RTW_ENTRY_GROUP || E.bvh_root >= 0) return false;
    for (int k = 0; k < E.n_ops; ++k)
        if (E.op[k] != RTW_OP_FLIP) return false;
    return true;
}
void world_runs(work& w) {
    const rtw_scene_desc* d = w.d;
    std::vector<world_run>& runs = w.runs;
    w.entry_movers.assign(std::max(d->n_entries, 1), 0);
    for (int e = 0; e < d->n_entries; ++e) {
        const rtw_entry& E = d->entries[e];
        for (int i = E.first_prim; i < E.first_prim + E.n_prims; ++i)
            w.entry_movers[e] |= w.prims[i].type >= DP_MOVING_COMMON ? 1 : 0;
        const bool plain = ray_plain(E);
        if (plain && !runs.empty() && runs.back().entry < 0 &&
            runs.back().first_prim + runs.back().n_prims == E.first_prim) {
            runs.back().n_prims += E.n_prims;
            runs.back().movers |= w.entry_movers[e];
            continue;
        }
        runs.push_back(world_run{plain ? WORLD_RUN_PLAIN : e, E.first_prim, E.n_prims, w.entry_movers[e]});
    }
    // plain runs of y-only spheres -> ysphere_scan (static ones get dy = 0)
    for (world_run& R : runs) {
        if (R.entry != WORLD_RUN_PLAIN || R.n_prims < 2) continue;
        bool all = true;
        for (int i = R.first_prim; i < R.first_prim + R.n_prims && all; ++i)
            all = w.prims[i].type == DP_MOVING_COMMON_Y || (w.prims[i].type == RTW_PRIM_SPHERE && w.prims[i].p[1] != 0.0);
        if (!all) continue;
        R.entry = WORLD_RUN_YSPHERES;
        for (int i = R.first_prim; i < R.first_prim + R.n_prims; ++i)
            if (w.prims[i].type == RTW_PRIM_SPHERE) w.prims[i].p[5] = 0.0;
    }
}

// ysphere_scan's fp32 prefilter records (rtw_device.h): spheres of
// y-sphere runs whose centre (incl. motion) is within 2^8 and radius
// within 2^4 are filtered, others (the random_balls ground, r = 1000)
// carry r^2 = +inf and always take the fp64 test; the maxima over the
// filtered ones bound the prefilter's rounding error
// (the records of a run are interleaved pairwise, spheres
// first + 2p and first + 2p + 1 sharing the 16 floats at 8 (first + 2p),
// component c of member s at 2c + s; the last sphere of a run of odd
// length keeps the plain record {cx, cy, cz, dy, rr} in its own 8 floats,
// so every record stays inside its run's slots; kYsAhead + 2 spare
// records at the end, slack for the unpacked form's prefetch ring)
void ysphere_records(work& w) {
    w.ysph.assign(8 * (std::max<size_t>(w.prims.size(), 1) + kYsAhead + 2), 0.0f);
    float* const ysb = w.ysb;
    auto up = [](double v) {  // fp32 value >= v
        float f = (float)v;
        if ((double)f < v) f = std::nextafter(f, INFINITY);
        return f;
    };
    for (const world_run& R : w.runs) {
        if (R.entry != WORLD_RUN_YSPHERES) continue;
        for (int i = R.first_prim; i < R.first_prim + R.n_prims; ++i) {
            const rtw_prim& q = w.prims[i];
            const int k = i - R.first_prim;
            const bool lone = k == R.n_prims - 1 && (k & 1) == 0;
            float* const rec = w.ysph.data() + 8 * (size_t)(R.first_prim + (k & ~1)) + (k & 1);
            auto f = [rec, lone](int c) -> float& { return rec[lone ? c : 2 * c]; };
            const double dy = q.type == DP_MOVING_COMMON_Y ? q.p[5] : 0.0;
            f(0) = (float)q.p[0], f(1) = (float)q.p[1], f(2) = (float)q.p[2], f(3) = (float)dy;
            const bool small = std::fabs(q.p[0]) <= 256 && std::fabs(q.p[1]) <= 256 && std::fabs(dy) <= 256 &&
                               std::fabs(q.p[2]) <= 256 && std::fabs(q.p[3]) <= 16;
            if (!small) {
                f(4) = INFINITY;
                continue;
            }
            f(4) = (float)q.p[9];
            ysb[0] = std::max(ysb[0], up(std::fabs(q.p[0])));
            ysb[1] = std::max(ysb[1], up(std::fabs(q.p[1])));
            ysb[2] = std::max(ysb[2], up(std::fabs(dy)));
            ysb[3] = std::max(ysb[3], up(std::fabs(q.p[2])));
            ysb[4] = std::max(ysb[4], up(q.p[9]));
        }
    }
}

// World-BVH leaves reference entries; a plain one-prim entry's item is
// replaced by ~prim so the walk tests the prim without reading the entry.
int world_leaf_items(work& w) {
    const rtw_scene_desc* d = w.d;
    w.items.assign(d->bvh_items, d->bvh_items + d->n_bvh_items);
    w.world_node.assign(d->n_bvh_nodes, 0);
    if (d->world_bvh_root < 0) return RTW_OK;
    std::vector<int> todo{d->world_bvh_root};
    while (!todo.empty()) {
        const rtw_bvh_node& N = d->bvh_nodes[todo.back()];
        w.world_node[todo.back()] = 1;
        todo.pop_back();
        if (N.count == 0) {
            todo.push_back(N.left);
            todo.push_back(N.right);
            continue;
        }
        for (int k = N.left; k < N.left + N.count; ++k) {
            if (w.items[k] < 0 || w.items[k] >= d->n_entries)
                return rtw_fail(RTW_ERR_INVALID, "world bvh item out of range");
            const rtw_entry& E = d->entries[w.items[k]];
            if (ray_plain(E) && E.n_prims == 1) w.items[k] = ~E.first_prim;
        }
    }
    return RTW_OK;
}

// One box record {x0, x1, y0, y1, z0, z1, first rect (int)} from the six
// rects at prim i, when they are the hittable_list box's (+z, -z, +y, -y,
// +x, -x: XY at z1 and z0, XZ at y1 and y0, YZ at x1 and x0, each with the
// box's other two ranges) to the last bit; get(prim, k) = p[k] in the
// precision of out.  False if not such a box.
template <class Get, class T>
bool box_planes(const std::vector<rtw_prim>& prims, Get get, int i, T* out) {
    if (i < 0 || i + 6 > (int)prims.size()) return false;
    const int ty[6] = {RTW_PRIM_RECT_XY, RTW_PRIM_RECT_XY, RTW_PRIM_RECT_XZ,
                       RTW_PRIM_RECT_XZ, RTW_PRIM_RECT_YZ, RTW_PRIM_RECT_YZ};
    for (int j = 0; j < 6; ++j)
        if (prims[i + j].type != ty[j]) return false;
    const T x0 = get(i + 5, 4), x1 = get(i + 4, 4), y0 = get(i + 3, 4), y1 = get(i + 2, 4);
    const T z0 = get(i + 1, 4), z1 = get(i, 4);
    const T want[6][4] = {{x0, x1, y0, y1}, {x0, x1, y0, y1}, {x0, x1, z0, z1},
                          {x0, x1, z0, z1}, {y0, y1, z0, z1}, {y0, y1, z0, z1}};
    for (int j = 0; j < 6; ++j)
        for (int k = 0; k < 4; ++k)
            if (!(get(i + j, k) == want[j][k])) return false;
    out[0] = x0, out[1] = x1, out[2] = y0, out[3] = y1, out[4] = z0, out[5] = z1;
    int32_t f = i;
    std::memcpy(out + 6, &f, sizeof f);  // the first rect, in the record's seventh slot
    return true;
}

// Box items' planes (scene::boxes): one 64-B record per box item,
// {x0, x1, y0, y1, z0, z1, first rect (int)}, packed densely (the 400
// ground boxes of Book 2 in 25 KB), when every box item's six rects are
// the hittable_list box's (box_planes).  The device items then read
// RTW_ITEM_BOX | record (the fp32 copy likewise, fscene::boxes); otherwise
// no table, and the walks read the rects of RTW_ITEM_BOX | first rect.
// (box_table false, RTW_BOX_TABLE=0 at upload: no table, for tests of the
// rect path)
void box_table_and_items(work& w, bool box_table) {
    std::vector<int> slot_items;  // item slots of box items
    for (size_t k = 0; k < w.items.size(); ++k)
        if (box_table && w.items[k] >= 0 && (w.items[k] & RTW_ITEM_BOX)) slot_items.push_back((int)k);
    std::map<int, int> rec_of;
    for (int k : slot_items) {
        const int i = w.items[k] & RTW_ITEM_INDEX;
        if (rec_of.count(i)) continue;
        rec_of[i] = (int)w.box_firsts.size();
        w.box_firsts.push_back(i);
    }
    w.boxes64.assign(8 * w.box_firsts.size(), 0.0);
    bool ok = true;
    for (size_t b = 0; b < w.box_firsts.size() && ok; ++b)
        ok = box_planes(w.prims, [&](int q, int k) { return w.prims[q].p[k]; }, w.box_firsts[b],
                        w.boxes64.data() + 8 * b);
    if (!ok) {
        w.boxes64.clear();
        w.box_firsts.clear();
    } else {
        for (int k : slot_items) w.items[k] = RTW_ITEM_BOX | rec_of[w.items[k] & RTW_ITEM_INDEX];
    }
}

// Inner BVH nodes: the axis along which their children's centres differ
// most, and whether the left child is the upper one (push_children).
void split_axes(work& w) {
    const rtw_scene_desc* d = w.d;
    w.nodes.assign(d->bvh_nodes, d->bvh_nodes + d->n_bvh_nodes);
    for (rtw_bvh_node& N : w.nodes) {
        N.pad = 0;
        if (N.count > 0) continue;
        const rtw_bvh_node& L = d->bvh_nodes[N.left];
        const rtw_bvh_node& R = d->bvh_nodes[N.right];
        int ax = 0;
        double best = -1.0;
        for (int k = 0; k < 3; ++k) {
            const double gap = std::fabs((R.bmin[k] + R.bmax[k]) - (L.bmin[k] + L.bmax[k]));
            if (gap > best) best = gap, ax = k;
        }
        const bool left_upper = (L.bmin[ax] + L.bmax[ax]) > (R.bmin[ax] + R.bmax[ax]);
        N.pad = ax | (left_upper ? 4 : 0);
    }
}

// fp32 device nodes (rtw_layout.h bvh_node32): bounds rounded outward;
// a BVH whose bounds are not finite within 2^90 is not used at all (the
// flat list gives the same image).
// The fp32 kernels' copy of the nodes (nodes32f): a one-item leaf holds its
// item (entry, ~prim, prim or box) in a instead of its index into the item
// array (b = -1), and a two-item group leaf holds both (a, and b =
// INT_MIN | second; b in [-16, -2] stays an index and a count), so the
// fp32 walks (rtw_fast.h) reach the prims with one dependent load less
// per leaf.  Measured (1 MI355X, A/B; bit-identical): C3 fp32 +1.9 %
// (profiles/r06/ab_r6r_C3f.log, parity_r6r_inl2.log), C5 fp32 +0.5 % for
// the group pairs (ab_r6t_C5f.log, parity_r6t_pair.log).  The fp64 walks
// keep the shared form: inline leaves there measured C3 -0.7 %
// (ab_r6r_C3.log).
void device_nodes(work& w) {
    w.nodes32.resize(w.nodes.size());
    w.nodes32f.resize(w.nodes.size());
    w.bvh_ok = w.nodes.size() < (1u << 28);
    for (size_t k = 0; k < w.nodes.size(); ++k) {
        const rtw_bvh_node& N = w.nodes[k];
        bvh_node32& M = w.nodes32[k];
        for (int j = 0; j < 3; ++j) {
            w.bvh_ok = w.bvh_ok && std::isfinite(N.bmin[j]) && std::isfinite(N.bmax[j]) &&
                       std::fabs(N.bmin[j]) <= 0x1p90 && std::fabs(N.bmax[j]) <= 0x1p90;
            float lo = (float)N.bmin[j], hi = (float)N.bmax[j];
            if ((double)lo > N.bmin[j]) lo = std::nextafter(lo, -INFINITY);
            if ((double)hi < N.bmax[j]) hi = std::nextafter(hi, INFINITY);
            M.lo[j] = lo, M.hi[j] = hi;
            w.bvh_bound = std::max(w.bvh_bound, std::max(std::fabs((double)lo), std::fabs((double)hi)));
        }
        M.a = N.left;
        M.b = N.count > 0 ? -N.count : (N.right | (N.pad << 28));
        w.nodes32f[k] = M;
        if (N.count == 1) w.nodes32f[k].a = w.items[N.left];
        // a group leaf's two items (prims or boxes: >= 0) in a and b's low bits
        if (!w.world_node[k] && N.count == 2 && w.items[N.left] >= 0 && w.items[N.left + 1] >= 0 &&
            w.items[N.left + 1] < 0x7fffffef) {
            w.nodes32f[k].a = w.items[N.left];
            w.nodes32f[k].b = (int32_t)(0x80000000u | (uint32_t)w.items[N.left + 1]);
        }
    }
}

// Breadth-first numbering from all roots together (the world BVH's, then
// every group's, in entry order): nodes [0, k) are then the top levels of
// every tree, the node packet the persistent BVH kernels stage in LDS.
void bfs_renumber(work& w) {
    w.entries.assign(w.d->entries, w.d->entries + w.d->n_entries);
    w.world_root = w.d->world_bvh_root;
    if (w.nodes32.empty()) return;
    std::vector<int> order, newid(w.nodes32.size(), -1);
    order.reserve(w.nodes32.size());
    auto enqueue = [&](int n) {
        if (n >= 0 && newid[n] < 0) newid[n] = (int)order.size(), order.push_back(n);
    };
    enqueue(w.world_root);
    for (const rtw_entry& E : w.entries) enqueue(E.bvh_root);
    for (size_t q = 0; q < order.size(); ++q) {
        const rtw_bvh_node& N = w.nodes[order[q]];
        if (N.count == 0) enqueue(N.left), enqueue(N.right);
    }
    for (size_t n = 0; n < w.nodes32.size(); ++n) enqueue((int)n);  // unreachable nodes keep a slot
    auto renumber = [&](std::vector<bvh_node32>& nodes) {
        std::vector<bvh_node32> bfs(nodes.size());
        for (size_t n = 0; n < nodes.size(); ++n) {
            bvh_node32 M = nodes[n];
            if (M.b >= 0) {  // inner: renumber both children, keep the split bits
                M.a = newid[M.a];
                M.b = newid[M.b & 0x0fffffff] | (M.b & ~0x0fffffff);
            }
            bfs[newid[n]] = M;
        }
        nodes.swap(bfs);
    };
    renumber(w.nodes32);
    renumber(w.nodes32f);
    if (w.world_root >= 0) w.world_root = newid[w.world_root];
    for (rtw_entry& E : w.entries)
        if (E.bvh_root >= 0) E.bvh_root = newid[E.bvh_root];
}

// device entries (dev_entry) and their op pool
void entries_and_ops(work& w) {
    w.dev_entries.resize(std::max<size_t>(w.entries.size(), 1));
    for (size_t e = 0; e < w.entries.size(); ++e) {
        const rtw_entry& E = w.entries[e];
        dev_entry& D = w.dev_entries[e];
        std::memset(&D, 0, sizeof D);
        D.kind = E.kind, D.first_prim = E.first_prim, D.n_prims = E.n_prims, D.n_ops = E.n_ops;
        D.first_op = (int32_t)w.dev_ops.size();
        D.phase_material = E.phase_material, D.bvh_root = E.bvh_root, D.n_outer_ops = E.n_outer_ops;
        D.movers = w.entry_movers[e];
        // the reference's -(1 / density), once per upload (a correctly
        // rounded division and a negation, as on the device)
        D.neg_inv_density = E.kind == RTW_ENTRY_MEDIUM ? -(1.0 / E.density) : 0.0;
        for (int k = 0; k < E.n_ops; ++k) {
            dev_op o;
            std::memset(&o, 0, sizeof o);
            o.type = E.op[k];
            for (int j = 0; j < 3; ++j) o.p[j] = E.op_param[k][j];
            w.dev_ops.push_back(o);
        }
    }
}

// The facts of the desc itself, and the refusal of a BVH too deep.
// BVH stack depth: a walk pushes two children per inner node and pops
// one, so it holds at most depth + 1 entries; a group BVH inside a world
// leaf stacks on top of the world walk.
int desc_facts(const work& w, layout_facts& f) {
    const rtw_scene_desc* d = w.d;
    f.features = (w.has_media ? F_MEDIA : 0) | (w.bvh_ok && d->world_bvh_root >= 0 ? F_WBVH : 0);
    for (int e = 0; e < d->n_entries; ++e)
        if (w.bvh_ok && d->entries[e].bvh_root >= 0) f.features |= F_GBVH;
    f.n_runs = (int)w.runs.size();
    for (const world_run& R : w.runs) {
        f.n_ysph_runs += R.entry == WORLD_RUN_YSPHERES;
        f.n_plain_runs += R.entry == WORLD_RUN_PLAIN;
    }
    f.ysph = f.n_ysph_runs > 0;
    for (int k = 0; k < d->n_prims; ++k) f.movers = f.movers || d->prims[k].type == RTW_PRIM_MOVING_SPHERE;
    for (int k = 0; k < d->n_materials; ++k) {
        const int t = d->materials[k].type;
        f.shade_mask |= t == RTW_MAT_METAL ? SF_METAL : t == RTW_MAT_DIELECTRIC ? SF_DIEL : t == RTW_MAT_ISOTROPIC ? SF_ISO : 0;
    }
    for (int k = 0; k < d->n_textures; ++k) {
        const int t = d->textures[k].type;
        f.shade_mask |= t == RTW_TEX_NOISE ? SF_NOISE : t == RTW_TEX_CHECKER ? SF_CHECKER : t == RTW_TEX_IMAGE ? SF_IMAGE : 0;
    }
    auto depth = [&](int root) {
        int best = 0;
        std::vector<std::pair<int, int>> todo{{root, 1}};
        while (!todo.empty()) {
            const auto [n, dd] = todo.back();
            todo.pop_back();
            best = std::max(best, dd);
            const rtw_bvh_node& N = d->bvh_nodes[n];
            if (N.count == 0) todo.push_back({N.left, dd + 1}), todo.push_back({N.right, dd + 1});
        }
        return best;
    };
    // A walk from an empty stack that pops one node and pushes both children
    // of an inner one holds at most D entries for a tree of depth D (the
    // entry at stack position j has depth >= j + 1: true for the root at 0,
    // and an inner node of depth k popped from position k' <= k - 1 puts
    // depth-(k + 1) children at k' and k' + 1).  The fp32 media kernel's
    // group walks are such walks (select_fp32).
    for (int e = 0; e < d->n_entries; ++e)
        if (d->entries[e].bvh_root >= 0) f.group_depth = std::max(f.group_depth, depth(d->entries[e].bvh_root));
    const int world_depth = d->world_bvh_root >= 0 ? depth(d->world_bvh_root) : 0;
    f.stack_need = world_depth + f.group_depth + 2;
    f.n_nodes = w.bvh_ok ? (int)w.nodes32.size() : 0;
    f.lights = d->n_lights > 0;
    f.black = d->background != RTW_BG_GRADIENT && d->render_type != RTW_RENDER_NORMAL;
    f.desc_pin = camera_is_pinhole(d->camera);
    f.bvh_motion = f.movers && d->n_bvh_nodes > 0;
    f.shutter0 = std::min(d->camera.time0, d->camera.time1);
    f.shutter1 = std::max(d->camera.time0, d->camera.time1);
    if (f.stack_need > kStack)
        return rtw_fail(RTW_ERR_UNSUPPORTED, "BVH too deep for the traversal stack (" + std::to_string(f.stack_need) +
                                                 " > " + std::to_string(kStack) + " entries)");
    return RTW_OK;
}

void scene_scalars(const work& w, const layout_facts& f, layout_scalars& s) {
    const rtw_scene_desc* d = w.d;
    s.bvh_bound = w.bvh_bound;
    s.ysb_cx = w.ysb[0], s.ysb_cy = w.ysb[1], s.ysb_dy = w.ysb[2], s.ysb_cz = w.ysb[3], s.ysb_r2 = w.ysb[4];
    s.n_runs = (int32_t)w.runs.size();
    s.mv_common = w.mv_common ? 1 : 0;
    s.mv_t0 = w.mv_t0;
    s.mv_den = w.mv_den;
    // walk_quot (rtw_device.h): every prim coordinate and radius within 2^40,
    // every mover on the common interval
    bool bounded = true;
    auto in = [&](double v) { return std::isfinite(v) && std::fabs(v) <= 0x1p40; };
    for (const rtw_prim& q : w.prims) {
        if (q.type == RTW_PRIM_MOVING_SPHERE) bounded = false;
        const int np = is_sphere(q.type) ? (q.type == RTW_PRIM_SPHERE ? 4 : 7) : 5;
        for (int k = 0; k < np; ++k) bounded = bounded && in(q.p[k]);
    }
    s.fast_div = bounded ? 1 : 0;
    s.n_entries = d->n_entries;
    s.n_lights = d->n_lights;
    s.light_weight = d->n_lights > 0 ? 1.0 / (double)d->n_lights : 0.0;
    s.world_bvh_root = w.bvh_ok ? w.world_root : -1;
    s.n_nodes = f.n_nodes;
    s.render_type = d->render_type;
    s.background = d->background;
    s.n_media = (int32_t)w.media.size();
    s.has_media = w.has_media ? 1 : 0;
    s.f_mv_t0 = (float)s.mv_t0;
    s.f_mv_inv_den = (float)(1.0 / s.mv_den);
    s.f_light_weight = (float)s.light_weight;
}

// The fp64 blob.  The arrays shading reads come first (layout_arrays64).
void pack64(const work& w, scene_layout& L) {
    const rtw_scene_desc* d = w.d;
    std::vector<char>& m = L.mem64;
    layout_arrays64& a = L.at64;
    a.prims = put(m, w.prims);
    a.entries = put(m, w.dev_entries.data(), sizeof(dev_entry) * (size_t)d->n_entries);
    a.materials = put(m, d->materials, sizeof(rtw_material) * d->n_materials);
    a.textures = put(m, d->textures, sizeof(rtw_texture) * d->n_textures);
    a.lights = put(m, d->lights, sizeof(rtw_light) * d->n_lights);
    a.ranvec = put(m, d->perlin_ranvec, d->has_perlin ? sizeof(double) * 768 : 0);
    a.perm = put(m, d->perlin_perm, d->has_perlin ? sizeof(int32_t) * 768 : 0);
    a.media = put(m, w.media);
    a.prim_onb = put(m, w.frames);
    a.mat_aux = put(m, w.mat_aux);
    a.ops = put(m, w.dev_ops);
    a.nodes = put(m, w.nodes32);
    a.items = put(m, w.items);
    a.runs = put(m, w.runs);
    a.ysph = put(m, w.ysph);
    a.boxes = put(m, w.boxes64);
    a.texels = put(m, d->image_texels, (size_t)d->image_bytes);
    if (m.size() < 256) m.resize(256, 0);
    L.facts.shade_bytes = (uint32_t)a.nodes.off;
}

// fp32 mirror for the fast mode (rtw_fast.h): prims, entries, ops,
// materials, textures, Perlin vectors and rect frames in single
// precision; BVH nodes / items, world runs, the media walk and the lights
// are the fp64 blob's arrays.
struct mirror {
    std::vector<prim32> prims;
    std::vector<ent32> entries;
    std::vector<op32> ops;
    std::vector<mat32> materials;
    std::vector<tex32> textures;
    std::vector<float> boxes, ranvec, frames;
};
int fp32_mirror(const work& w, mirror& m) {
    const rtw_scene_desc* d = w.d;
    m.prims.resize(std::max(d->n_prims, 1));
    for (int i = 0; i < d->n_prims; ++i) {
        const rtw_prim& q = d->prims[i];
        prim32& o = m.prims[i];
        std::memset(&o, 0, sizeof o);
        o.type = q.type, o.material = q.material, o.flip = q.flip, o.entry = q.entry;
        for (int k = 0; k < 10; ++k) o.p[k] = (float)q.p[k];
        if (is_sphere(q.type)) {
            o.p[9] = (float)(q.p[3] * q.p[3]);
            if (q.type == RTW_PRIM_MOVING_SPHERE) {
                for (int k = 0; k < 3; ++k) o.p[4 + k] = (float)(q.p[4 + k] - q.p[k]);
                o.p[7] = (float)q.p[7];
                o.p[8] = (float)(1.0 / (q.p[8] - q.p[7]));
            }
        }
    }
    m.entries.resize(std::max(d->n_entries, 1));
    for (int e = 0; e < d->n_entries; ++e) {
        const dev_entry& D = w.dev_entries[e];
        ent32& o = m.entries[e];
        std::memset(&o, 0, sizeof o);
        o.kind = D.kind, o.first_prim = D.first_prim, o.n_prims = D.n_prims, o.n_ops = D.n_ops;
        o.first_op = D.first_op, o.phase_material = D.phase_material;
        o.bvh_root = w.bvh_ok ? D.bvh_root : -1;
        o.n_outer_ops = D.n_outer_ops;
        o.neg_inv_density = (float)D.neg_inv_density;
    }
    m.ops.resize(std::max<size_t>(w.dev_ops.size(), 1));
    for (size_t k = 0; k < w.dev_ops.size(); ++k) {
        m.ops[k].type = w.dev_ops[k].type;
        for (int j = 0; j < 3; ++j) m.ops[k].p[j] = (float)w.dev_ops[k].p[j];
    }
    m.materials.resize(std::max(d->n_materials, 1));
    for (int k = 0; k < d->n_materials; ++k) {
        const rtw_material& M = d->materials[k];
        mat32& o = m.materials[k];
        std::memset(&o, 0, sizeof o);
        o.type = M.type, o.texture = M.texture;
        for (int j = 0; j < 3; ++j) o.albedo[j] = (float)M.albedo[j];
        o.fuzz = (float)M.fuzz, o.ref_idx = (float)M.ref_idx;
        o.inv_ref_idx = (float)w.mat_aux[2 * k], o.r0 = (float)w.mat_aux[2 * k + 1];
    }
    m.textures.resize(std::max(d->n_textures, 1));
    for (int k = 0; k < d->n_textures; ++k) {
        const rtw_texture& T = d->textures[k];
        tex32& o = m.textures[k];
        std::memset(&o, 0, sizeof o);
        o.type = T.type, o.odd = T.odd, o.even = T.even, o.scale = (float)T.scale;
        o.offset = T.offset;  // RTW_TEX_IMAGE: odd / even = nx / ny, texels at S.texels + offset
        for (int j = 0; j < 3; ++j) o.color[j] = (float)T.color[j];
    }
    m.boxes.assign(8 * w.box_firsts.size(), 0.0f);  // the same records in fp32 (fscene::boxes)
    for (size_t b = 0; b < w.box_firsts.size(); ++b)
        if (!box_planes(w.prims, [&](int q, int k) { return m.prims[q].p[k]; }, w.box_firsts[b], m.boxes.data() + 8 * b))
            return rtw_fail(RTW_ERR_INVALID, "box planes: fp32 rects differ from the fp64 ones");
    m.ranvec.resize(d->has_perlin ? 768 : 0);
    m.frames.resize(w.frames.size());
    for (size_t k = 0; k < m.ranvec.size(); ++k) m.ranvec[k] = (float)d->perlin_ranvec[k];
    for (size_t k = 0; k < w.frames.size(); ++k) m.frames[k] = (float)w.frames[k];
    return RTW_OK;
}

// The fp32 blob: everything fp32 shading reads first (layout_arrays32).
void pack32(const work& w, const mirror& f, scene_layout& L) {
    const rtw_scene_desc* d = w.d;
    std::vector<char>& m = L.mem32;
    layout_arrays32& a = L.at32;
    a.prims = put(m, f.prims);
    a.entries = put(m, f.entries);
    a.ops = put(m, f.ops);
    a.materials = put(m, f.materials);
    a.textures = put(m, f.textures);
    a.ranvec = put(m, f.ranvec);
    a.frames = put(m, f.frames);
    a.lights = put(m, d->lights, sizeof(rtw_light) * d->n_lights);
    a.perm = put(m, d->perlin_perm, d->has_perlin ? sizeof(int32_t) * 768 : 0);
    // (after the staged prefix)
    a.nodes = put(m, w.nodes32f);
    a.boxes = put(m, f.boxes);
    if (m.size() < 256) m.resize(256, 0);
    L.facts.f32_bytes = (uint32_t)(a.perm.off + a.perm.bytes);
}

}  // namespace

int rtw_layout_scene(const rtw_scene_desc* d, bool box_table, scene_layout* out) {
    work w;
    w.d = d;
    scene_layout L;
    media_walk(w);
    frames_and_materials(w);
    prims_and_movers(w);
    world_runs(w);
    ysphere_records(w);
    if (int rc = world_leaf_items(w)) return rc;
    box_table_and_items(w, box_table);
    split_axes(w);
    device_nodes(w);
    bfs_renumber(w);
    entries_and_ops(w);
    if (int rc = desc_facts(w, L.facts)) return rc;
    scene_scalars(w, L.facts, L.s);
    mirror f32;
    if (int rc = fp32_mirror(w, f32)) return rc;
    pack64(w, L);
    pack32(w, f32, L);
    *out = std::move(L);
    return RTW_OK;
}

rtwd::select_in rtw_layout_select_in(const layout_facts& f, bool pin) {
    select_in s;
    s.features = f.features, s.shade_mask = f.shade_mask;
    s.shade_bytes = f.shade_bytes, s.f32_bytes = f.f32_bytes;
    s.stack_need = f.stack_need, s.group_depth = f.group_depth, s.n_nodes = f.n_nodes;
    s.ysph = f.ysph, s.static_scene = !f.movers, s.lights = f.lights, s.black = f.black;
    s.pin = pin;
    return s;
}
