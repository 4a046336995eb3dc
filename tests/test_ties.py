"""The test scenes of the equal-distance rule, on the CPU: "ties" holds a twin
pair -- identical geometry, different material -- of every category the
kernels decide separately, its BVHs split some pairs across leaves and keep
some together, every pair has power (the oracle's render changes visibly when
the two exchange places), and on every station of "ties_axis" the rect wins.

hittable_list::hit keeps the last rect among equal t (a rect accepts
t == t_max), the first sphere (t < t_max), and a rect over a sphere.  The
oracle is pinned to the reference's own renders of "ties" bit for bit
(tests/test_oracle.py, tests/golden/render_ties_*.npy); "ties_axis" needs a
camera the reference's camera class cannot construct and is tied to the
oracle only."""
import functools

import numpy as np
import pytest

import bvh_forms as bf
import ties
from oracle_lib import finalize_np, oracle_sums
from raytracingweekend_amd import _abi

TOL = 1e-4  # the project's written tolerance (tests/test_gpu_parity.py)
SPHERES = (_abi.RTW_PRIM_SPHERE, _abi.RTW_PRIM_MOVING_SPHERE)
RECTS = (_abi.RTW_PRIM_RECT_XY, _abi.RTW_PRIM_RECT_XZ, _abi.RTW_PRIM_RECT_YZ)


@pytest.fixture(scope="module")
def api(built):
    from raytracingweekend_amd import render
    return render


@pytest.mark.parametrize("bvh", [False, True], ids=["flat", "bvh"])
def test_every_category_holds_a_twin_pair(api, bvh):
    sd = api.SceneDesc("ties", ties.ASPECT, use_bvh=bvh)
    d = sd.desc
    assert d.n_entries == ties.N_ENTRIES and d.n_lights == 0 and d.background == _abi.RTW_BG_GRADIENT
    assert not any(d.entries[e].kind == _abi.RTW_ENTRY_MEDIUM for e in range(d.n_entries))
    units = ties.twin_units(d)  # asserts same geometry and different material for a..f
    assert set(units) == {"a", "b", "c", "c'", "d", "e", "f", "g", "h"}
    P, E = d.prims, d.entries

    def first(cat, k=0):
        return units[cat][k][0]

    # a: static sphere twins off y = 0, adjacent plain entries (a y-sphere run); b: on y = 0
    for cat, on_y0 in (("a", False), ("b", True)):
        i, j = first(cat)
        assert P[i].type == P[j].type == _abi.RTW_PRIM_SPHERE and (P[i].p[1] == 0.0) == on_y0
        assert P[i].p[3] == -P[j].p[3] and P[i].p[9] == P[j].p[9]
        assert j == i + 1 and E[P[i].entry].n_ops == E[P[j].entry].n_ops == 0
    # c: y-only movers on the common interval, x and z nonzero; c': x-movers
    for cat, axis in (("c", 1), ("c'", 0)):
        i, j = first(cat)
        assert P[i].type == P[j].type == _abi.RTW_PRIM_MOVING_SPHERE
        assert (P[i].p[7], P[i].p[8]) == (0.0, 1.0) and P[i].p[0] != 0.0 and P[i].p[2] != 0.0
        moved = [P[i].p[4 + a] != P[i].p[a] for a in range(3)]
        assert moved == [a == axis for a in range(3)]
        assert P[i].p[3] == -P[j].p[3]
    # d, f: the twins lie in different entries, exactly one of them with ops; both list orders
    for cat, types in (("d", SPHERES), ("f", RECTS)):
        assert len(units[cat]) == 2
        ops_first = []
        for unit in units[cat]:
            (i, j), = unit
            assert P[i].type in types and P[i].entry != P[j].entry
            na, nb = E[P[i].entry].n_ops, E[P[j].entry].n_ops
            assert (na > 0) != (nb > 0)
            ops_first.append(na > 0)
        assert sorted(ops_first) == [False, True]
    assert {P[first("f", k)[0]].type for k in range(2)} == {_abi.RTW_PRIM_RECT_YZ, _abi.RTW_PRIM_RECT_XZ}
    # the zero transforms are exact: offset 0, sin 0, cos 1
    for e in range(d.n_entries):
        for k in range(E[e].n_ops):
            if e in (ties.GROUPS["g"], ties.GROUPS["h"]):
                continue
            prm = tuple(E[e].op_param[k])
            assert prm == ((0.0, 0.0, 0.0) if E[e].op[k] == _abi.RTW_OP_TRANSLATE else (0.0, 1.0, 0.0))
    # e: coincident xy_rects and a third rect over a part of them
    i, j = first("e")
    third = P[j + 1]
    assert P[i].type == P[j].type == third.type == _abi.RTW_PRIM_RECT_XY and third.p[4] == P[i].p[4]
    assert P[i].flip & 1 != P[j].flip & 1
    assert P[i].p[0] < third.p[0] < P[i].p[1] < third.p[1] and P[i].p[2] < third.p[2] < P[i].p[3] < third.p[3]
    # g, h: translated lists of at least ten items holding five twin pairs each
    G, H = E[ties.GROUPS["g"]], E[ties.GROUPS["h"]]
    assert G.n_ops == 1 and G.n_prims == 11 and len(units["g"]) == 5
    assert H.n_ops == 1 and H.n_prims == 66 and len(units["h"]) == 5
    assert all(P[i].type == _abi.RTW_PRIM_SPHERE for u in units["g"] for i, _ in u)
    assert all(P[i].type in RECTS for u in units["h"] for i, _ in u)
    # wherever the class allows it the twins differ in normal as well
    for cat, us in units.items():
        for unit in us:
            for i, j in unit:
                if P[i].type in SPHERES:
                    assert P[i].p[3] == -P[j].p[3]
                else:
                    flips = [(P[q].flip + sum(E[P[q].entry].op[k] == _abi.RTW_OP_FLIP
                                              for k in range(E[P[q].entry].n_ops))) & 1 for q in (i, j)]
                    assert flips[0] != flips[1], (cat, i, j)
    if not bvh:
        assert d.world_bvh_root < 0 and d.n_bvh_nodes == 0
        return
    assert d.world_bvh_root >= 0 and G.bvh_root >= 0 and H.bvh_root >= 0
    assert all(E[e].bvh_root < 0 for e in range(d.n_entries) if e not in ties.GROUPS.values())
    items = lambda root: [d.bvh_items[k] for n in bf.subtree(d, root) if d.bvh_nodes[n].count > 0
                          for k in range(d.bvh_nodes[n].left, d.bvh_nodes[n].left + d.bvh_nodes[n].count)]
    assert sorted(items(G.bvh_root)) == list(range(G.first_prim, G.first_prim + G.n_prims))
    assert sorted(items(H.bvh_root)) == [_abi.RTW_ITEM_BOX | i for i in range(H.first_prim, H.first_prim + H.n_prims, 6)]


def _leaf_of(d, root):
    """{item (a box item without its flag): the leaf node holding it}."""
    out = {}
    for n in bf.subtree(d, root):
        nd = d.bvh_nodes[n]
        for k in range(nd.left, nd.left + nd.count if nd.count > 0 else nd.left):
            out[d.bvh_items[k] & _abi.RTW_ITEM_INDEX if d.bvh_items[k] & _abi.RTW_ITEM_BOX else d.bvh_items[k]] = n
    return out


def _shared_and_split(d):
    units = ties.twin_units(d)
    shared = split = 0
    for cat in ("g", "h"):
        leaf = _leaf_of(d, d.entries[ties.GROUPS[cat]].bvh_root)
        for unit in units[cat]:
            i, j = unit[0]  # a prim item, or the first rect of a box item
            shared += leaf[i] == leaf[j]
            split += leaf[i] != leaf[j]
    return shared, split


def test_leaf_sizes_split_and_share_twin_pairs(api, monkeypatch):
    """Twins in two leaves are arbitrated across leaves, in whatever order the
    walk reaches them; twins in one leaf within the leaf's item loop."""
    d = api.SceneDesc("ties", ties.ASPECT, use_bvh=True).desc
    group, world = bf.leaf_sizes(d)
    assert max(group) <= 2 and max(world) == 1  # the default leaf sizes
    shared, split = _shared_and_split(d)
    assert split >= 1, "no g or h twin pair is split across two leaves under the default leaf sizes"
    bf.set_leaf_env(monkeypatch, 16, 16)
    d16 = api.SceneDesc("ties", ties.ASPECT, use_bvh=True).desc
    group, world = bf.leaf_sizes(d16)
    assert max(group) > 2 and max(world) > 1
    shared16, _ = _shared_and_split(d16)
    assert shared16 >= 1, "no g or h twin pair shares a leaf under leaf sizes 16, 16"
    # the world twins (d, f) share a world leaf there as well
    wleaf = _leaf_of(d16, d16.world_bvh_root)
    assert any(wleaf[ea] == wleaf[eb] for cat in ("d", "f") for ea, eb in ties.PAIRS[cat])


@functools.lru_cache(maxsize=None)
def _oracle_ties():
    from raytracingweekend_amd import render
    nx, ny, spp, depth = ties.SIZE
    sd = render.SceneDesc("ties", ties.ASPECT)
    sums, seg = oracle_sums(sd, nx, ny, spp, depth, seed=41)
    sums.setflags(write=False)
    return sd, sums, seg


UNIT_IDS = [(cat, k) for cat, n in (("a", 1), ("b", 1), ("c", 1), ("c'", 1), ("d", 2), ("e", 1), ("f", 2), ("g", 5),
                                    ("h", 5)) for k in range(n)]


@pytest.mark.parametrize("cat,k", UNIT_IDS, ids=[f"{c}{k}" for c, k in UNIT_IDS])
def test_every_twin_pair_has_power(api, cat, k):
    """A condition on the scene, with no mutated code: with one pair's twins
    exchanged (material and flip, so the other one wins every tie between
    them) the oracle's canvas moves by more than the tolerance of the GPU
    tests in at least 8 pixels, and the traversal count changes.  A kernel
    that picks the wrong twin of this pair renders the exchanged scene."""
    nx, ny, spp, depth = ties.SIZE
    sd, base, seg = _oracle_ties()
    unit = ties.twin_units(sd.desc)[cat][k]
    other, seg_other = oracle_sums(ties.exchanged(sd, unit), nx, ny, spp, depth, seed=41)
    moved = np.abs(finalize_np(other, spp) - finalize_np(base, spp)).reshape(-1, 3).max(axis=1) > TOL
    print(f"TIES power {cat}{k}: {int(moved.sum())} pixels move, traversals {seg} -> {seg_other}")
    assert moved.sum() >= 8
    assert seg_other != seg


@pytest.mark.parametrize("station", range(len(ties.STATIONS)))
def test_the_rect_wins_on_every_axis_station(api, station):
    nx, ny = ties.AXIS_SIZE
    spp = 2
    sd = api.SceneDesc("ties_axis", 1.0)
    d = sd.desc
    assert d.n_entries > 8
    S = ties.STATIONS[station]
    sphere, winner = ties.station_prim(d, S["sphere"]), ties.station_prim(d, S["winner"])
    assert d.prims[sphere].type == _abi.RTW_PRIM_SPHERE and d.prims[winner].type == _abi.RTW_PRIM_RECT_XY
    # the touching point in small integers: centre z - 5, radius 1, the rect's plane z = -4, in the station's frame
    x = 10.0 * station - sum(d.entries[S["sphere"][0]].op_param[k][0] for k in range(d.entries[S["sphere"][0]].n_ops))
    assert tuple(d.prims[sphere].p[:4]) == (x, 0.0, -5.0, 1.0)
    wide = 8.0 if station == 4 else 0.0
    assert tuple(d.prims[winner].p[:5]) == (x - 1.0, x + 1.0 + wide, -1.0, 1.0, -4.0) and d.prims[winner].flip & 1
    e = d.entries[S["winner"][0]]
    rects = [q for q in range(e.first_prim, e.first_prim + e.n_prims) if d.prims[q].type == _abi.RTW_PRIM_RECT_XY]
    assert winner == rects[-1], "the winner is the station's last rect"
    cam = ties.station_camera(station)
    normals, seg = oracle_sums(ties.normal_desc(sd), nx, ny, spp, 50, seed=3, camera=cam)
    assert seg == nx * ny * spp
    assert np.array_equal(normals.reshape(-1, 3), np.tile(np.multiply(ties.WINNER_NORMAL, spp), (nx * ny, 1)))
    shaded, seg = oracle_sums(sd, nx, ny, spp, 50, seed=3, camera=cam)
    assert seg == nx * ny * spp, "the winner emits and scatters nothing"
    assert np.array_equal(shaded.reshape(-1, 3), np.tile(np.multiply(S["emits"], spp), (nx * ny, 1)))
    # the sphere with the winner's material: the same render (the sphere is never the hit)
    cp = bf.DescCopy(sd)
    cp.own_prims()[sphere].material = d.prims[winner].material
    same, seg = oracle_sums(cp, nx, ny, spp, 50, seed=3, camera=cam)
    assert np.array_equal(same, shaded) and seg == nx * ny * spp
    # with BVHs the desc holds a world BVH over the stations
    assert api.SceneDesc("ties_axis", 1.0, use_bvh=True).desc.world_bvh_root >= 0


@pytest.mark.parametrize("bvh", [False, True], ids=["flat", "bvh"])
def test_prim_ranges_must_ascend_with_the_entry_index(api, bvh):
    """Two entries with their prim ranges exchanged are the same list -- the
    oracle, which walks entries, renders the same image -- but prim index
    order is no longer list order, by which the BVH walks decide hits at equal
    distance: validate_desc refuses the desc (before any device is asked for)."""
    nx, ny, spp, depth = 24, 16, 2, 50
    sd = api.SceneDesc("ties", ties.ASPECT, use_bvh=bvh)
    cp = ties.permuted_ranges(sd, *ties.PAIRS["d"][0])
    a, sa = oracle_sums(sd, nx, ny, spp, depth, seed=2)
    b, sb = oracle_sums(cp, nx, ny, spp, depth, seed=2)
    assert sa == sb and np.array_equal(a, b)
    rc, msg = bf.upload_status(cp.desc)
    assert rc == -5 and "prim ranges must ascend with the entry index" in msg, (rc, msg)  # RTW_ERR_UNSUPPORTED
