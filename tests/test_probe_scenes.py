"""The probe scenes (probe_scene, csrc/host/scenes.cpp; rendered by
tests/test_gpu_fp32_probes.py): every kind flattens, flat and with BVHs, the
desc holds the feature the kind is there for, and validate_desc accepts it.
No GPU here."""
import ctypes as C
import math

import pytest

from raytracingweekend_amd import _abi

KINDS = ["rect_light", "sphere_light", "far_sphere_light", "default_light", "glass", "metal", "medium", "motion",
         "textures"]
ASPECT = 64 / 48


@pytest.fixture(scope="module")
def descs(built):
    from raytracingweekend_amd.render import SceneDesc
    return {(k, bvh): SceneDesc("probe_" + k, ASPECT, use_bvh=bvh) for k in KINDS for bvh in (False, True)}


def _prims(d):
    return [d.prims[i] for i in range(d.n_prims)]


def _spheres(d):
    return [q for q in _prims(d) if q.type == _abi.RTW_PRIM_SPHERE]


def _light_prims(d, kind):
    return [d.prims[d.lights[i].prim] for i in range(d.n_lights) if d.lights[i].kind == kind]


def _materials(d, type_):
    return [d.materials[i] for i in range(d.n_materials) if d.materials[i].type == type_]


def _texture_types(d):
    return {d.textures[i].type for i in range(d.n_textures)}


@pytest.mark.parametrize("bvh", [False, True], ids=["flat", "bvh"])
@pytest.mark.parametrize("kind", KINDS)
def test_validate_desc_accepts_the_probe(descs, kind, bvh):
    # validate_desc is the check rtw_scene_upload runs first; the library
    # exports it for the host check programs (rtw_host_util.h), as a C++ symbol
    validate = getattr(_abi.lib(), "_Z13validate_descPK14rtw_scene_desc")
    validate.restype, validate.argtypes = C.c_int, [C.POINTER(_abi.rtw_scene_desc)]
    sd = descs[kind, bvh]
    assert validate(sd.ptr) == 0, _abi.lib().rtw_last_error().decode()
    d = sd.desc
    assert d.n_prims > 0 and d.n_entries > 0 and d.render_type == _abi.RTW_RENDER_SHADED
    # use_bvh builds something in every kind: a world BVH, or a group's
    group_roots = [d.entries[i].bvh_root for i in range(d.n_entries) if d.entries[i].bvh_root >= 0]
    if bvh:
        assert d.n_bvh_nodes > 0 and (d.world_bvh_root >= 0 or group_roots)
    else:
        assert d.n_bvh_nodes == 0 and d.world_bvh_root < 0 and not group_roots


def test_unknown_probe_kind_is_no_scene(built):
    p = C.POINTER(_abi.rtw_scene_desc)()
    for name in ("probe_", "probe_nothing", "probe_glass "):
        assert _abi.lib().rtw_scene_builtin(name.encode(), ASPECT, 0, C.byref(p)) != 0 and not p


@pytest.mark.parametrize("bvh", [False, True], ids=["flat", "bvh"])
class TestFeatures:
    def test_rect_light_is_long_flipped_and_the_only_light(self, descs, bvh):
        d = descs["rect_light", bvh].desc
        assert d.background == _abi.RTW_BG_BLACK and d.n_lights == 1
        (q,) = _light_prims(d, _abi.RTW_LIGHT_XZ_RECT)
        sides = sorted([q.p[1] - q.p[0], q.p[3] - q.p[2]])
        assert sides[0] > 0 and sides[1] / sides[0] >= 3
        # the world's copy of the lamp is flipped, and so is the lit surface
        world = [w for w in _prims(d)[:d.n_prims - 1] if w.type == _abi.RTW_PRIM_RECT_XZ and w.entry >= 0]
        lamp = [w for w in world if list(w.p)[:5] == list(q.p)[:5]]
        assert lamp and all(w.flip for w in lamp)
        assert any(d.entries[i].n_ops >= 2 for i in range(d.n_entries))  # translate(rotate_y(box))

    def test_default_light_has_a_member_without_a_pdf(self, descs, bvh):
        d = descs["default_light", bvh].desc
        kinds = [d.lights[i].kind for i in range(d.n_lights)]
        assert kinds == [_abi.RTW_LIGHT_XZ_RECT, _abi.RTW_LIGHT_DEFAULT]
        assert d.lights[1].prim < 0

    def test_sphere_light_subtends_ten_to_eighty_degrees(self, descs, bvh):
        d = descs["sphere_light", bvh].desc
        (q,) = _light_prims(d, _abi.RTW_LIGHT_SPHERE)
        assert q.type == _abi.RTW_PRIM_SPHERE and q.p[3] < 0  # emits outwards (sphere.h:71-77)
        r, h = abs(q.p[3]), q.p[1]  # above the floor y == 0
        half = lambda x: math.degrees(math.asin(r / math.hypot(x, h)))
        assert half(0.0) >= 75 and half(6.0) <= 10.5

    def test_far_sphere_light_is_a_thousandth_of_its_distance(self, descs, bvh):
        d = descs["far_sphere_light", bvh].desc
        assert d.n_lights == 1 and d.background == _abi.RTW_BG_BLACK
        (q,) = _light_prims(d, _abi.RTW_LIGHT_SPHERE)
        dist = math.sqrt(q.p[0] ** 2 + q.p[1] ** 2 + q.p[2] ** 2)  # from the floor's centre, the origin
        assert abs(q.p[3]) / dist <= 1 / 500
        floor = [w for w in _prims(d) if w.type == _abi.RTW_PRIM_RECT_XZ and w.p[4] == 0.0 and w.p[0] == -w.p[1]]
        assert floor

    def test_glass_has_a_hollow_shell(self, descs, bvh):
        d = descs["glass", bvh].desc
        assert d.background == _abi.RTW_BG_GRADIENT and d.n_lights == 0
        glass = {i for i in range(d.n_materials) if d.materials[i].type == _abi.RTW_MAT_DIELECTRIC}
        radii = [q.p[3] for q in _spheres(d) if q.material in glass]
        assert any(r < 0 for r in radii) and sum(r > 0 for r in radii) >= 2

    def test_metal_has_the_three_fuzzes_and_a_rect(self, descs, bvh):
        d = descs["metal", bvh].desc
        metals = {i: d.materials[i].fuzz for i in range(d.n_materials) if d.materials[i].type == _abi.RTW_MAT_METAL}
        on_spheres = {metals[q.material] for q in _spheres(d) if q.material in metals}
        assert {0.0, 0.3, 1.0} <= on_spheres
        assert any(q.type == _abi.RTW_PRIM_RECT_XY and q.material in metals for q in _prims(d))

    def test_medium_has_two_media(self, descs, bvh):
        d = descs["medium", bvh].desc
        media = [d.entries[i] for i in range(d.n_entries) if d.entries[i].kind == _abi.RTW_ENTRY_MEDIUM]
        assert sorted(e.density for e in media) == [0.5, 2.0]
        assert any(e.n_ops >= 2 for e in media) and any(e.n_prims == 1 for e in media)
        assert len(_materials(d, _abi.RTW_MAT_ISOTROPIC)) == 2 and d.n_visits > 0

    def test_motion_has_every_mover_class(self, descs, bvh):
        d = descs["motion", bvh].desc
        movers = [q for q in _prims(d) if q.type == _abi.RTW_PRIM_MOVING_SPHERE]
        assert any(q.p[7] != 0 for q in movers), "a mover with time0 != 0"
        assert any(q.p[4] != q.p[0] for q in movers), "an x-mover"
        assert any(q.p[5] != q.p[1] and q.p[4] == q.p[0] for q in movers), "a y-mover"
        assert any(q.entry >= 0 and d.entries[q.entry].n_ops >= 1 for q in movers), "a translated mover"
        assert any(q.type == _abi.RTW_PRIM_MOVING_SPHERE for q in _light_prims(d, _abi.RTW_LIGHT_SPHERE))
        assert (d.camera.time0, d.camera.time1) == (0.0, 1.0)

    def test_textures_has_checker_marble_and_a_lens(self, descs, bvh):
        d = descs["textures", bvh].desc
        assert _texture_types(d) == {_abi.RTW_TEX_CONSTANT, _abi.RTW_TEX_CHECKER, _abi.RTW_TEX_NOISE}
        assert d.has_perlin and d.camera.lens_radius > 0
        assert any(q.p[3] == 1000.0 for q in _spheres(d))
