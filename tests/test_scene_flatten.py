"""The host scene API + flattener against dumps of the reference's own scene
graphs (tests/golden/scene_*.json, from oracle/_ref/rtw_ref).

Walks the reference tree the way the flattener is specified to (world list
order, transforms peeled outermost first, flips folded into primitives, boxes
and nested lists as groups) and requires every number to match exactly.
"""
import json
from pathlib import Path

import numpy as np
import pytest

from raytracingweekend_amd import _abi

GOLD = Path(__file__).resolve().parent / "golden"
SCENES = ["cornell_box", "random_balls", "dielectric", "light_sample", "book2_final"]
# the scene of coincident primitives, composed from the reference's classes in oracle/ref_harness.cpp
SCENES += ["ties"]
# the probe scenes, composed from the reference's classes in oracle/ref_harness.cpp
PROBES = ["probe_" + kind for kind in ("rect_light", "sphere_light", "far_sphere_light", "default_light", "glass",
                                       "metal", "medium", "motion", "textures")]

RECT = {"xy_rect": _abi.RTW_PRIM_RECT_XY, "xz_rect": _abi.RTW_PRIM_RECT_XZ, "yz_rect": _abi.RTW_PRIM_RECT_YZ}


def _leaves(node, flip, out):
    t = node["type"]
    if t in RECT:
        out.append((RECT[t], tuple(node["p"]), node["mat"], flip))
    elif t == "sphere":
        out.append((_abi.RTW_PRIM_SPHERE, tuple(node["center"]) + (node["radius"],), node["mat"], flip))
    elif t == "moving_sphere":
        out.append((_abi.RTW_PRIM_MOVING_SPHERE,
                    tuple(node["center"]) + (node["radius"],) + tuple(node["center1"]) + (node["time0"], node["time1"]),
                    node["mat"], flip))
    elif t == "flip":
        _leaves(node["ptr"], flip + 1, out)
    elif t == "box":
        _leaves(node["list"], flip, out)
    elif t == "list":
        for o in node["objects"]:
            _leaves(o, flip, out)
    else:
        raise AssertionError(f"unexpected node {t} inside a group")


def _entry(node):
    kind, density, phase = _abi.RTW_ENTRY_GROUP, 0.0, -1
    if node["type"] == "constant_medium":
        kind, density, phase = _abi.RTW_ENTRY_MEDIUM, node["density"], node["mat"]
        node = node["boundary"]
    ops = []
    while node["type"] in ("translate", "rotate_y"):
        if node["type"] == "translate":
            ops.append((_abi.RTW_OP_TRANSLATE, tuple(node["offset"])))
        else:
            ops.append((_abi.RTW_OP_ROTATE_Y, (node["sin"], node["cos"], 0.0)))
        node = node["ptr"]
    prims = []
    _leaves(node, 0, prims)
    return kind, density, phase, ops, prims


def _tex_content(dump, tid):
    t = dict(dump["textures"][tid])
    if t["type"] == "checker":  # texture.h:29-50: both children, by content
        t["odd"], t["even"] = _tex_content(dump, t["odd"]), _tex_content(dump, t["even"])
    return t


def _mat_content(dump, mid):
    m = dict(dump["materials"][mid])
    if "texture" in m:
        m["texture"] = _tex_content(dump, m["texture"])
    return m


def _desc_tex(desc, tid):
    t = desc.textures[tid]
    if t.type == _abi.RTW_TEX_CONSTANT:
        return {"type": "constant", "color": list(t.color)}
    if t.type == _abi.RTW_TEX_NOISE:
        return {"type": "noise", "scale": t.scale}
    assert t.type == _abi.RTW_TEX_CHECKER
    return {"type": "checker", "odd": _desc_tex(desc, t.odd), "even": _desc_tex(desc, t.even)}


def _desc_mat(desc, mid):
    m = desc.materials[mid]
    names = {0: "lambertian", 1: "metal", 2: "dielectric", 3: "diffuse_light", 4: "isotropic"}
    out = {"type": names[m.type]}
    if m.type == _abi.RTW_MAT_METAL:
        out["albedo"], out["fuzz"] = list(m.albedo), m.fuzz
    elif m.type == _abi.RTW_MAT_DIELECTRIC:
        out["ref_idx"] = m.ref_idx
    else:
        out["texture"] = _desc_tex(desc, m.texture)
    return out


@pytest.fixture(scope="module")
def render_mod(built):
    from raytracingweekend_amd import render
    return render


@pytest.mark.parametrize("name", SCENES + PROBES)
def test_flattened_scene_equals_reference_graph(render_mod, name):
    dump = json.loads((GOLD / f"scene_{name}.json").read_text())
    sd = render_mod.SceneDesc(name, dump["aspect"])
    d = sd.desc
    world = dump["world"]["objects"]
    assert d.n_entries == len(world)
    pi = 0
    for ei, node in enumerate(world):
        kind, density, phase, ops, prims = _entry(node)
        e = d.entries[ei]
        assert e.kind == kind and e.n_ops == len(ops) and e.n_prims == len(prims) and e.first_prim == pi
        if kind == _abi.RTW_ENTRY_MEDIUM:
            assert e.density == density
            assert _desc_mat(d, e.phase_material) == _mat_content(dump, phase)
        for k, (op, prm) in enumerate(ops):
            assert e.op[k] == op
            assert tuple(e.op_param[k][:3]) == prm[:3] if op == _abi.RTW_OP_TRANSLATE else \
                tuple(e.op_param[k][:2]) == prm[:2]
        for typ, p, mat, flip in prims:
            q = d.prims[pi]
            assert q.type == typ and q.entry == ei and (q.flip & 1) == (flip & 1)
            assert tuple(q.p[:len(p)]) == p
            assert _desc_mat(d, q.material) == _mat_content(dump, mat)
            pi += 1
    # lights (Scene/scene.h:269 lights list)
    lights = dump["lights"]["objects"] if dump["lights"] else []
    assert d.n_lights == len(lights)
    # "light_pdf" is present where a member samples with hittable's defaults
    # (hittable.h:36-37: pdf_value 0, random (1, 0, 0)); the classes with a pdf
    # of their own are xz_rect and sphere_base
    own_pdf = dump.get("light_pdf", ["own"] * len(lights))
    assert len(own_pdf) == len(lights)
    for li, node in enumerate(lights):
        L = d.lights[li]
        want = {"xz_rect": _abi.RTW_LIGHT_XZ_RECT, "sphere": _abi.RTW_LIGHT_SPHERE,
                "moving_sphere": _abi.RTW_LIGHT_SPHERE}.get(node["type"], _abi.RTW_LIGHT_DEFAULT)
        assert node["type"] != "unknown"
        assert (want == _abi.RTW_LIGHT_DEFAULT) == (own_pdf[li] == "default")
        assert L.kind == want
        if want != _abi.RTW_LIGHT_DEFAULT:
            # a prim of the light's own, in no world entry: a member that is
            # only a light (probe_motion's moving sphere) is hit by no ray
            q = d.prims[L.prim]
            assert q.entry == -1 and L.prim >= pi
            if node["type"] == "xz_rect":
                assert q.type == _abi.RTW_PRIM_RECT_XZ and tuple(q.p[:5]) == tuple(node["p"])
            elif node["type"] == "sphere":
                assert q.type == _abi.RTW_PRIM_SPHERE
                assert tuple(q.p[:4]) == tuple(node["center"]) + (node["radius"],)
            else:  # sphere.h:20-38: the whole movement, pdf_value's hit evaluates it
                assert q.type == _abi.RTW_PRIM_MOVING_SPHERE
                assert tuple(q.p[:9]) == (tuple(node["center"]) + (node["radius"],) + tuple(node["center1"]) +
                                          (node["time0"], node["time1"]))
            assert _desc_mat(d, q.material) == _mat_content(dump, node["mat"])
    # camera (camera.h:13-34)
    cam = dump["camera"]
    c = d.camera
    for k in ("origin", "lower_left", "horizontal", "vertical", "u", "v", "w"):
        assert tuple(getattr(c, k)) == tuple(cam[k]), k
    assert (c.time0, c.time1, c.lens_radius) == (cam["time0"], cam["time1"], cam["lens_radius"])
    assert d.background == (_abi.RTW_BG_GRADIENT if dump["background"] == "gradient" else _abi.RTW_BG_BLACK)
    assert d.render_type == _abi.RTW_RENDER_SHADED


def test_random_balls_layout(render_mod):
    """485 objects from the default-seeded engine; the
    right-to-left argument order of g++ decides which jitter is x."""
    sd = render_mod.SceneDesc("random_balls", 1.5)
    assert sd.desc.n_entries == 485


def test_bvh_build_is_well_formed(render_mod):
    for name in ("random_balls", "book2_final"):
        sd = render_mod.SceneDesc(name, 1.0, use_bvh=True)
        d = sd.desc
        items = [d.bvh_items[i] for i in range(d.n_bvh_items)]
        roots = []
        if d.world_bvh_root >= 0:
            roots.append(("world", d.world_bvh_root, d.n_entries))
        for ei in range(d.n_entries):
            if d.entries[ei].bvh_root >= 0:
                roots.append((ei, d.entries[ei].bvh_root, None))
        assert roots
        for tag, root, n in roots:
            seen = []
            stack = [root]
            while stack:
                nd = d.bvh_nodes[stack.pop()]
                assert all(nd.bmin[a] <= nd.bmax[a] for a in range(3))
                if nd.count > 0:
                    seen += items[nd.left:nd.left + nd.count]
                else:
                    stack += [nd.left, nd.right]
            if tag == "world":
                assert sorted(seen) == list(range(n))
            else:
                # box items (RTW_ITEM_BOX | i) stand for the six rects [i, i+6)
                e = d.entries[tag]
                prims = []
                for it in seen:
                    if it & _abi.RTW_ITEM_BOX:
                        i = it & _abi.RTW_ITEM_INDEX
                        assert [d.prims[i + j].type for j in range(6)] == [_abi.RTW_PRIM_RECT_XY] * 2 + \
                            [_abi.RTW_PRIM_RECT_XZ] * 2 + [_abi.RTW_PRIM_RECT_YZ] * 2
                        prims += range(i, i + 6)
                    else:
                        prims.append(it)
                assert sorted(prims) == list(range(e.first_prim, e.first_prim + e.n_prims))
                if name == "book2_final" and e.n_prims == 2400:  # the 400 ground boxes
                    assert sum(1 for it in seen if it & _abi.RTW_ITEM_BOX) == 400


def _depth(d, root):
    best, todo = 0, [(root, 1)]
    while todo:
        n, k = todo.pop()
        best = max(best, k)
        if d.bvh_nodes[n].count == 0:
            todo += [(d.bvh_nodes[n].left, k + 1), (d.bvh_nodes[n].right, k + 1)]
    return best


@pytest.mark.parametrize("seed", range(4))
def test_group_walk_stack_depth_bound(render_mod, seed):
    """The fp32 media kernel sizes its LDS stacks by the deepest group BVH
    (rtw_select.h kMediaStack, select_fp32): a walk from an
    empty stack that pops one node and pushes both children of an inner one
    never holds more than D entries for a tree of depth D.  Replays that walk
    (rtw_fast.h group_bvh pushes right, then left; the fp64 walks push the
    nearer child last, so the order here is also drawn at random) on Book 2's
    group trees, with slab tests passing at random and always, and checks the
    bound is never passed; Book 2's trees fit the 12-entry stacks."""
    import random
    rnd = random.Random(seed)
    d = render_mod.SceneDesc("book2_final", 1.0, use_bvh=True).desc
    roots = [d.entries[e].bvh_root for e in range(d.n_entries) if d.entries[e].bvh_root >= 0]
    assert d.world_bvh_root < 0 and len(roots) == 2
    for root in roots:
        D = _depth(d, root)
        assert D <= 12
        for p_pass in (1.0, 0.7, 0.4):
            for shuffled in (False, True):
                sp_max, stack = 0, [root]
                while stack:
                    nd = d.bvh_nodes[stack.pop()]
                    if p_pass < 1.0 and rnd.random() > p_pass:
                        continue
                    if nd.count == 0:
                        kids = [nd.right, nd.left]
                        if shuffled and rnd.random() < 0.5:
                            kids.reverse()
                        stack += kids
                        sp_max = max(sp_max, len(stack))
                assert sp_max <= D


def test_unknown_scene_is_an_error(render_mod):
    from raytracingweekend_amd import RtwError
    with pytest.raises(RtwError, match="unknown scene"):
        render_mod.SceneDesc("no_such_scene", 1.0)
