"""Helpers of the equal-distance tests (test_ties.py on the CPU,
test_gpu_ties.py on the GPU): where the twins of the "ties" scene lie in its
flattened desc, copies of the desc with one twin pair exchanged, and the
station cameras of "ties_axis" (csrc/host/scenes.cpp says what both scenes
hold).  No tests here."""
from __future__ import annotations

import bvh_forms as bf
from raytracingweekend_amd import _abi

SIZE = (48, 32, 4, 50)  # nx, ny, spp, depth of the reference's renders of "ties"
ASPECT = 48 / 32

# world entries of the twin pairs, per category, and the two groups
# (ties_scene's Add order; test_ties.py checks every one against the desc)
PAIRS = {"a": [(1, 2)], "c": [(3, 4)], "d": [(5, 6), (7, 8)], "b": [(9, 10)], "c'": [(11, 12)], "e": [(13, 14)],
         "f": [(16, 17), (18, 19)]}
GROUPS = {"g": 20, "h": 21}
N_ENTRIES = 22


def same_geometry(a, b):
    """Equal type and parameters; a sphere's radius may differ in sign (the
    same radius^2: the same roots)."""
    if a.type != b.type:
        return False
    pa, pb = list(a.p), list(b.p)
    if a.type in (_abi.RTW_PRIM_SPHERE, _abi.RTW_PRIM_MOVING_SPHERE):
        pa[3], pb[3] = abs(pa[3]), abs(pb[3])
    return pa == pb


def twin_units(d):
    """{category: [unit]}: a unit is the list of (i, j) prim index pairs, i <
    j, exchanged together -- one pair, or the six face pairs of twin boxes.
    Twins are a Lambertian and a metal primitive of the same geometry (the
    third coincident item of g and of h is glass)."""
    def is_twin(i, j):
        kinds = {d.materials[d.prims[q].material].type for q in (i, j)}
        return same_geometry(d.prims[i], d.prims[j]) and kinds == {_abi.RTW_MAT_LAMBERTIAN, _abi.RTW_MAT_METAL}

    out = {}
    for cat, pairs in PAIRS.items():
        out[cat] = []
        for ea, eb in pairs:
            A, B = d.entries[ea], d.entries[eb]
            assert A.n_prims == 1 and B.n_prims == 1
            assert is_twin(A.first_prim, B.first_prim), (cat, ea, eb)
            out[cat].append([(A.first_prim, B.first_prim)])
    for cat, stride in (("g", 1), ("h", 6)):  # items: prims, or boxes of six rects
        E = d.entries[GROUPS[cat]]
        starts = range(E.first_prim, E.first_prim + E.n_prims, stride)
        out[cat] = [[(i + f, j + f) for f in range(stride)] for i in starts for j in starts
                    if i < j and all(is_twin(i + f, j + f) for f in range(stride))]
    return out


def exchanged(sd, unit):
    """A DescCopy of `sd` in which the twins of `unit` have exchanged their
    material and flip: the same scene with the two in the other list order."""
    cp = bf.DescCopy(sd)
    prims = cp.own_prims()
    for i, j in unit:
        prims[i].material, prims[j].material = prims[j].material, prims[i].material
        prims[i].flip, prims[j].flip = prims[j].flip, prims[i].flip
    return cp


def permuted_ranges(sd, ea, eb):
    """A DescCopy of `sd` in which entries `ea` and `eb` (one prim each) have
    exchanged their prim ranges: the same list of objects, but the later
    entry's prim now has the lower index."""
    cp = bf.DescCopy(sd)
    prims, entries = cp.own_prims(), cp.own_entries()
    a, b = entries[ea], entries[eb]
    assert a.n_prims == 1 and b.n_prims == 1
    ia, ib = a.first_prim, b.first_prim
    keep = _abi.rtw_prim.from_buffer_copy(prims[ia])
    prims[ia] = _abi.rtw_prim.from_buffer_copy(prims[ib])
    prims[ib] = keep
    a.first_prim, b.first_prim = ib, ia
    prims[ib].entry, prims[ia].entry = ea, eb
    return cp


# ---- "ties_axis" ------------------------------------------------------------
# per station: (entry, offset in the entry) of its sphere and of its winning
# rect, and the winner's emission
STATIONS = [
    {"sphere": (0, 0), "winner": (1, 0), "emits": (0.5, 1.0, 0.25)},
    {"sphere": (3, 0), "winner": (2, 0), "emits": (1.0, 0.25, 0.5)},
    {"sphere": (5, 0), "winner": (6, 0), "emits": (0.25, 0.5, 1.0)},
    {"sphere": (7, 1), "winner": (7, 2), "emits": (2.0, 0.5, 0.125)},
    {"sphere": (9, 0), "winner": (8, 0), "emits": (0.125, 2.0, 1.0)},  # the wide rect, reached second by a BVH walk
]
WINNER_NORMAL = (0.5, 0.5, 0.0)  # 0.5 (n + 1) of the flipped rect's (0, 0, -1)
LOSER_NORMAL = (0.5, 0.5, 1.0)   # the sphere's and the unflipped rect's (0, 0, 1)
AXIS_SIZE = (8, 8)


def station_camera(k):
    """Every primary ray is exactly origin (10 k, 0, 0), direction (0, 0, -1)."""
    x = 10.0 * k
    cam = _abi.rtw_camera_desc()
    cam.origin[:] = (x, 0.0, 0.0)
    cam.lower_left[:] = (x, 0.0, -1.0)
    cam.horizontal[:] = (0.0, 0.0, 0.0)
    cam.vertical[:] = (0.0, 0.0, 0.0)
    cam.u[:], cam.v[:], cam.w[:] = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    cam.time0, cam.time1, cam.lens_radius = 0.0, 1.0, 0.0
    return cam


def station_prim(d, where):
    e, k = where
    return d.entries[e].first_prim + k


def normal_desc(sd):
    cp = bf.DescCopy(sd)
    cp.desc.render_type = _abi.RTW_RENDER_NORMAL
    return cp
