"""The BVH kernels and leaf forms no built-in scene reaches by default, and
RTW_RENDER_NORMAL, on the GPU.

* Normal mode (0.5 (n + 1) at the first hit, one traversal per sample): fp64
  against the oracle's Normal render (itself pinned to the reference's,
  test_oracle.py), on list, world-BVH, group-BVH and media scenes.
* Leaf forms: with RTW_BVH_LEAF_MAX / RTW_BVH_WORLD_LEAF_MAX at (5, 3) and
  (16, 16) the walks decode leaves of 3..16 items; the fp64 BVH render equals
  the flat render bit for bit (test_gpu_parity.py's invariant).
* Private traversal stacks: Book 2 with one-item leaves (fp32), and a
  hand-built deep world BVH over random_balls (fp64 and fp32); a deeper one
  is refused.
* fp32 has no sample-exact reference, and its slab test is not provably
  conservative against fp32 hit distances, so renders over different trees
  need not agree bit for bit.  Its check is the statistic of test_gpu_fp32.py
  (tests/fp32_stats.py) on Normal-mode renders against the oracle's: a
  Normal-mode sample has only jitter noise, so a skipped, duplicated or
  misread leaf item shows as a bias many times the noise.  Curved scenes
  only (a block inside one flat wall has no jitter variance).  Beside it,
  the fp32 render over each tree may differ from the one over the default
  tree (same seed) in a handful of pixels at most.

Every case prints the kernels rtw_scene_query reports (pytest -s)."""
import functools

import numpy as np
import pytest

import bvh_forms as bf
import fp32_stats
from oracle_lib import finalize_np, oracle_sums
from raytracingweekend_amd import _abi
from raytracingweekend_amd._abi import RtwError
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

F_MEDIA, F_WBVH, F_GBVH = 1, 2, 4  # rtw_select.h


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


def _normal(sd):
    sd.desc.render_type = _abi.RTW_RENDER_NORMAL
    return sd


def _report(case, info):
    print(f"KERNELS {case}: fp64 {info['kernel']} | fp32 {info['kernel_fast']} | features {info['features']}")


@functools.lru_cache(maxsize=None)
def _oracle_normal(scene, nx, ny, spp, seed):
    """The oracle's Normal render of the flat scene (computed once per case,
    shared by the flat and BVH cases and by every tree of the fp32 checks)."""
    from raytracingweekend_amd import render
    ref, seg = oracle_sums(_normal(render.SceneDesc(scene, nx / ny)), nx, ny, spp, 50, seed=seed)
    ref.setflags(write=False)
    return ref, seg


@functools.lru_cache(maxsize=None)
def _flat_render(scene, nx, ny, spp, seed):
    """The fp64 render of the flat scene on the GPU (shared by every tree
    compared with it)."""
    from raytracingweekend_amd import render
    ds = render.DeviceScene(render.SceneDesc(scene, nx / ny))
    try:
        acc, st = ds.render_accumulate(nx, ny, spp, 50, seed=seed)
    finally:
        ds.close()
    acc.setflags(write=False)
    return acc, st["segments"]


@functools.lru_cache(maxsize=None)
def _fast_default(scene, nx, ny, spp):
    """The fp32 Normal render over the default tree, first fast seed (call
    with the leaf-size environment unset)."""
    from raytracingweekend_amd import render
    ds = render.DeviceScene(_normal(render.SceneDesc(scene, nx / ny, use_bvh=True)))
    try:
        acc, _ = ds.render_accumulate(nx, ny, spp, 50, seed=fp32_stats.FAST_SEEDS[0], precision="fp32")
    finally:
        ds.close()
    acc.setflags(write=False)
    return acc


# ---- Normal mode, fp64 against the oracle ----------------------------------
NORMAL_CASES = [
    # scene, nx, ny, spp, use_bvh
    ("cornell_box", 32, 32, 4, False),
    ("random_balls", 48, 32, 4, False),
    ("random_balls", 48, 32, 4, True),
    ("nested", 48, 36, 4, False),
    ("book2_final", 24, 24, 2, False),
    ("book2_final", 24, 24, 2, True),
    ("textured", 48, 32, 4, False),
    ("textured", 48, 32, 4, True),
    ("grouped", 48, 32, 4, False),
    ("grouped", 48, 32, 4, True),
    ("grouped_world", 48, 32, 4, False),
    ("grouped_world", 48, 32, 4, True),
]


@pytest.mark.parametrize("scene,nx,ny,spp,bvh", NORMAL_CASES,
                         ids=[f"{c[0]}{'_bvh' if c[4] else ''}" for c in NORMAL_CASES])
def test_normal_mode_matches_oracle(gpu, scene, nx, ny, spp, bvh):
    ds = gpu.DeviceScene(_normal(gpu.SceneDesc(scene, nx / ny, use_bvh=bvh)))
    try:
        acc, st = ds.render_accumulate(nx, ny, spp, 50, seed=7)
        _report(f"normal {scene} bvh={bvh}", ds.query())
    finally:
        ds.close()
    ref, seg = _oracle_normal(scene, nx, ny, spp, 7)
    assert st["samples"] == nx * ny * spp
    assert st["segments"] == nx * ny * spp and seg == nx * ny * spp
    c_gpu, c_ref = finalize_np(acc, spp), finalize_np(ref, spp)
    assert np.all(np.isfinite(c_gpu))
    d = np.abs(c_gpu - c_ref)
    assert d.max() <= TOL, f"max per-channel diff {d.max()} at {np.argmax(d)}"


@pytest.mark.parametrize("scene,want", [("grouped", F_GBVH), ("grouped_world", F_WBVH | F_GBVH)])
def test_grouped_scenes_select_group_bvh_kernels(gpu, scene, want):
    """The kernels of the two test scenes carry F_GBVH without F_MEDIA (and
    F_WBVH for grouped_world), in both precisions; their walks fit the LDS
    stacks."""
    import re
    ds = gpu.DeviceScene(gpu.SceneDesc(scene, 1.5, use_bvh=True))
    try:
        info = ds.query()
    finally:
        ds.close()
    _report(f"shaded {scene} bvh=True", info)
    assert info["features"] & (F_MEDIA | F_WBVH | F_GBVH) == want
    for name, family in ((info["kernel"], "k_persist<"), (info["kernel_fast"], "k_fast<")):
        assert name.startswith(family) and name.endswith("true>"), name
        assert int(re.match(r"\w+<(\d+)", name).group(1)) & (F_MEDIA | F_WBVH | F_GBVH) == want, name


# ---- leaf forms, fp64: the BVH render equals the flat render ----------------
LEAF_SCENES = [("random_balls", 96, 64), ("book2_final", 48, 48), ("nested_plain", 48, 36),
               ("grouped_world", 48, 36)]


@pytest.mark.parametrize("env", bf.LEAF_ENVS, ids=lambda e: f"leaf{e[0]}_{e[1]}")
@pytest.mark.parametrize("scene,nx,ny", LEAF_SCENES, ids=[c[0] for c in LEAF_SCENES])
def test_leaf_forms_equal_flat(gpu, monkeypatch, scene, nx, ny, env):
    bf.set_leaf_env(monkeypatch, *env)
    sd = gpu.SceneDesc(scene, nx / ny, use_bvh=True)
    bf.assert_leaf_forms(sd.desc, scene, env)
    ds = gpu.DeviceScene(sd)
    try:
        tree, st = ds.render_accumulate(nx, ny, 2, 50, seed=5)
        _report(f"leaves {env} {scene}", ds.query())
    finally:
        ds.close()
    flat, seg_flat = _flat_render(scene, nx, ny, 2, 5)
    assert st["segments"] == seg_flat
    assert np.array_equal(flat, tree), f"max diff {np.abs(flat - tree).max()}"


# ---- private traversal stacks ----------------------------------------------
DEEP_CHAIN = 20  # world depth 30, stack_need 32: past the 16 LDS entries, within the 48 private ones


def test_deep_world_bvh_takes_private_stacks_and_equals_flat(gpu):
    """A world BVH too deep for the LDS stacks: k_persist<..., false> and
    k_fast<..., false>; the fp64 render equals the flat render bit for bit."""
    nx, ny = 96, 64
    cp = bf.deep_world_bvh(gpu.SceneDesc("random_balls", nx / ny), DEEP_CHAIN)
    assert bf.LDS_STACK < bf.stack_need(cp.desc) <= bf.STACK_MAX
    ds = gpu.DeviceScene(cp)
    try:
        info = ds.query()
        _report("deep world BVH random_balls", info)
        assert info["kernel"].startswith("k_persist<") and info["kernel"].endswith("false>"), info["kernel"]
        assert info["kernel_fast"].startswith("k_fast<") and info["kernel_fast"].endswith("false>"), info
        assert info["features"] & (F_MEDIA | F_WBVH | F_GBVH) == F_WBVH
        tree, st = ds.render_accumulate(nx, ny, 2, 50, seed=5)
    finally:
        ds.close()
    flat, seg_flat = _flat_render("random_balls", nx, ny, 2, 5)
    assert st["segments"] == seg_flat
    assert np.array_equal(flat, tree), f"max diff {np.abs(flat - tree).max()}"


def test_too_deep_world_bvh_is_refused(gpu):
    """stack_need > 48: rtw_scene_upload refuses the scene (nothing is
    launched: there is no handle to render with)."""
    cp = bf.deep_world_bvh(gpu.SceneDesc("random_balls", 1.5), 60)
    assert bf.stack_need(cp.desc) > bf.STACK_MAX
    with pytest.raises(RtwError, match=r"BVH too deep for the traversal stack \(\d+ > 48 entries\)"):
        gpu.DeviceScene(cp)


# ---- fp32: the statistic on Normal-mode renders ------------------------------
def _tree(gpu, monkeypatch, scene, tree, aspect):
    """The scene desc of a named tree."""
    if tree == "deep":
        return bf.deep_world_bvh(gpu.SceneDesc(scene, aspect), DEEP_CHAIN)
    if tree == "leaf1":
        monkeypatch.setenv("RTW_BVH_LEAF_MAX", "1")
    elif tree != "default":
        bf.set_leaf_env(monkeypatch, *[int(v) for v in tree[4:].split("_")])
    return gpu.SceneDesc(scene, aspect, use_bvh=True)


FP32_SCENES = ("random_balls", "book2_final", "grouped_world")
FP32_CASES = [(s, "default") for s in FP32_SCENES]  # first: a failure here is about the fp32 first hit itself
FP32_CASES += [(s, f"leaf{a}_{b}") for a, b in bf.LEAF_ENVS for s in FP32_SCENES]
FP32_CASES += [("book2_final", "leaf1"), ("random_balls", "deep")]


@pytest.mark.parametrize("scene,tree", FP32_CASES, ids=[f"{s}-{t}" for s, t in FP32_CASES])
def test_fast_mode_first_hits_are_statistically_the_oracles(gpu, monkeypatch, scene, tree):
    nx, ny, spp = 96, 64, 8
    sd = _normal(_tree(gpu, monkeypatch, scene, tree, nx / ny))
    monkeypatch.undo()  # the flattener has read the leaf sizes
    if tree.startswith("leaf") and tree != "leaf1":
        bf.assert_leaf_forms(sd.desc, scene, tuple(int(v) for v in tree[4:].split("_")))
    ds = gpu.DeviceScene(sd)
    try:
        info = ds.query()
        _report(f"fp32 normal {scene} {tree}", info)
        fast, other = fp32_stats.render_sets(ds, nx, ny, spp, 50)
    finally:
        ds.close()
    assert info["kernel_fast"].startswith("k_fast<")
    if tree in ("leaf1", "deep"):
        assert info["kernel_fast"].endswith("false>"), info["kernel_fast"]
    else:
        assert info["kernel_fast"].endswith("true>"), info["kernel_fast"]
    for acc, st in fast + other:
        assert st["samples"] == nx * ny * spp and st["segments"] == nx * ny * spp
        assert np.all(np.isfinite(acc))
    ref, _ = _oracle_normal(scene, nx, ny, spp, fp32_stats.REF_SEED)
    figures = fp32_stats.assert_statistically_the_reference([a for a, _ in fast], [a for a, _ in other], ref,
                                                            nx, ny, spp)
    print(f"FP32STAT {scene} {tree}: {figures}")
    if tree != "default":
        # Same seed, same draws: the two fp32 renders differ only where a slab
        # test at a node face culled a hit in one tree and not in the other.
        # Bit-identity is not asserted (the fp32 slab test allows 2 ulp and is
        # not provably conservative); the figure is printed, and bounded,
        # because the statistic above is weak on Book 2: with every third
        # sphere of its cluster dropped (another sphere of the clump takes
        # its place, with a normal as random) the oracle's renders still pass
        # it at this size, while 159 of the 6144 pixels change.  A grazing
        # miss needs a ray within a few fp32 ulp of a node face that also
        # bounds its hit: under 1e-4 of the samples by a wide margin, so
        # under 8 * 6144 * 1e-4 = 5 pixels; the bound is three times that.
        dflt = _fast_default(scene, nx, ny, spp)
        differ = int((dflt.reshape(-1, 3) != fast[0][0].reshape(-1, 3)).any(axis=1).sum())
        print(f"FP32TREES {scene} {tree}: {differ} of {nx * ny} pixels differ from the default tree's render")
        assert differ <= 15, f"{differ} pixels differ from the default tree's fp32 render"
