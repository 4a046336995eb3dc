"""The fp32 fast mode against the fp64 mode on converged renders of the probe
scenes (probe_scene, csrc/host/scenes.cpp): one shading feature per scene, so
an error in one device function is not diluted by a whole frame of everything
else, and enough samples that every pixel carries a standard error of a
fraction of a per cent (tests/fp32_converged.py has the rules and where the
multipliers come from).

Per probe kind, flat and with BVHs:

* the fp64 mode is tied to the oracle sample for sample, as
  tests/test_gpu_parity.py does for the built-in scenes (canvas within its
  TOL, equal traversal counts): the reference of the comparison below is the
  reference's arithmetic on this scene too;
* 64x48, depth 50, spp = 2^k in 16 sample-range chunks into one pair of moment
  buffers: fp64 seed 1, fp64 seed 2, fp32 seed 3 (another seed on purpose:
  both modes start a sample's stream from the same state).  The control
  compares the two fp64 renders without the floor; then fp32 is compared with
  fp64 seed 1.  k is the smallest at which the power condition holds on the
  fp64 render, measured once and fixed in K below.

With `pytest -s` every case prints the row recorded in
profiles/fp32_probes/results.txt.
"""
import time

import numpy as np
import pytest

import fp32_converged as fc
from oracle_lib import finalize_np, oracle_sums
from raytracingweekend_amd import _abi
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

NX, NY, DEPTH = 64, 48, 50
SEED_REF, SEED_CONTROL, SEED_FAST = 1, 2, 3
NARROW = (0.25, 0.5)  # a shutter inside the motion scene's [0, 1]

# (scene, bvh, shutter) -> k, spp = 2^k: the smallest k with power on the fp64
# render (profiles/fp32_probes/results.txt has the figures at k)
K = {
    ("probe_rect_light", False, None): 16, ("probe_rect_light", True, None): 16,
    ("probe_sphere_light", False, None): 16, ("probe_sphere_light", True, None): 16,
    ("probe_far_sphere_light", False, None): 16, ("probe_far_sphere_light", True, None): 16,
    ("probe_default_light", False, None): 15, ("probe_default_light", True, None): 15,
    ("probe_glass", False, None): 11, ("probe_glass", True, None): 11,
    ("probe_metal", False, None): 11, ("probe_metal", True, None): 11,
    ("probe_medium", False, None): 13, ("probe_medium", True, None): 13,
    ("probe_motion", False, None): 14, ("probe_motion", True, None): 14,
    ("probe_motion", False, NARROW): 14, ("probe_motion", True, NARROW): 14,
    ("probe_textures", False, None): 14, ("probe_textures", True, None): 14,
    # No built-in scene rides along: cornell_box (flat) and book2_final (BVH)
    # have no power at k = 16 (median se / m 1.0 % and 3.5 %; results.txt).
}
CASES = list(K)


def case_id(case):
    scene, bvh, shutter = case
    return scene.replace("probe_", "") + ("-bvh" if bvh else "-flat") + ("-narrow" if shutter else "")


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


def camera_of(sd, shutter):
    """The scene's camera, or a copy with a narrower shutter."""
    if shutter is None:
        return None
    cam = _abi.rtw_camera_desc.from_buffer_copy(sd.camera)
    cam.time0, cam.time1 = shutter
    return cam


def render_chunked(ds, spp, seed, precision, camera=None):
    """One render of spp samples per pixel as fc.CHUNKS equal sample ranges
    into one pair of moment buffers; every chunk's traversal count is kept."""
    assert spp % fc.CHUNKS == 0
    s1 = np.zeros(NX * NY * 3)
    s2 = np.zeros_like(s1)
    per = spp // fc.CHUNKS
    segments, samples = [], []
    for c in range(fc.CHUNKS):
        _, _, st = ds.render_moments(NX, NY, spp, DEPTH, seed, spp_begin=c * per, spp_count=per, accum=s1,
                                     accum_sq=s2, camera=camera, precision=precision)
        segments.append(st["segments"])
        samples.append(st["samples"])
    assert sum(samples) == NX * NY * spp
    assert np.all(np.isfinite(s1)) and np.all(np.isfinite(s2))
    return fc.Render(S1=s1, S2=s2, n=spp, segments=segments, samples=samples)


def converged_case(gpu, case, k):
    """The three renders of a case at spp = 2^k and both comparisons.
    Returns (info, power figures, control Result, fp32 Result, seconds);
    raises fc.NoPower where the fp64 render is too noisy at this k."""
    scene, bvh, shutter = case
    sd = gpu.SceneDesc(scene, NX / NY, use_bvh=bvh)
    ds = gpu.DeviceScene(sd)
    t0 = time.perf_counter()
    try:
        info = ds.query()
        cam = camera_of(sd, shutter)
        ref = render_chunked(ds, 1 << k, SEED_REF, "fp64", cam)
        pw = fc.power(ref, NX, NY)
        control = render_chunked(ds, 1 << k, SEED_CONTROL, "fp64", cam)
        fast = render_chunked(ds, 1 << k, SEED_FAST, "fp32", cam)
    finally:
        ds.close()
    return (info, pw, fc.compare(control, ref, NX, NY, 0.0), fc.compare(fast, ref, NX, NY),
            time.perf_counter() - t0)


def report(case, k, info, pw, control, test, seconds):
    print(f"\nPROBE {case_id(case):26s} k={k:2d}  {info['kernel']} | {info['kernel_fast']}  "
          f"level {pw['level']:.4f}  frame term {pw['frame_term']:.2e}  median se/m {pw['median_rel_se']:.2e}  "
          f"{seconds:.1f} s")
    print(f"PROBE   control {control.row()}  {control.failures or 'ok'}")
    print(f"PROBE   fp32    {test.row()}  {test.failures or 'ok'}")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fp64_mode_is_the_oracle_on_the_scene(gpu, case):
    scene, bvh, shutter = case
    spp = 4
    sd = gpu.SceneDesc(scene, NX / NY, use_bvh=bvh)
    ds = gpu.DeviceScene(sd)
    try:
        cam = camera_of(sd, shutter)
        acc, st = ds.render_accumulate(NX, NY, spp, DEPTH, SEED_REF, camera=cam)
    finally:
        ds.close()
    ref, seg = oracle_sums(sd, NX, NY, spp, DEPTH, SEED_REF, camera=cam)
    assert np.all(np.isfinite(acc)) and acc.sum() > 0
    assert np.abs(finalize_np(acc, spp) - finalize_np(ref, spp)).max() <= TOL
    assert st["segments"] == seg


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fast_mode_converges_to_the_fp64_mode(gpu, case):
    k = K[case]
    assert 4 <= k <= 16
    info, pw, control, test, seconds = converged_case(gpu, case, k)
    report(case, k, info, pw, control, test, seconds)
    assert info["kernel_fast"].startswith(("k_fast<", "k_fast_sort<"))
    # a control that fails means tails too heavy for this statistic: the
    # scene has to change, never the multipliers
    assert not control.failures, f"control: {control.failures}: {control.row()}\n  " + "\n  ".join(control.detail)
    assert not test.failures, f"fp32: {test.failures}: {test.row()}\n  " + "\n  ".join(test.detail)


def test_probes_reach_both_fast_kernels_with_and_without_media_and_group_bvhs(gpu):
    """Over the probe set: k_fast_sort and k_fast, each with and without
    F_MEDIA; k_fast with and without F_GBVH (feature bits: rtw_select.h; the
    kernel's first template argument)."""
    F_MEDIA, F_GBVH = 1, 4
    seen = set()
    for scene, bvh, shutter in CASES:
        if not scene.startswith("probe_") or shutter:
            continue
        ds = gpu.DeviceScene(gpu.SceneDesc(scene, NX / NY, use_bvh=bvh))
        try:
            name = ds.query()["kernel_fast"]
        finally:
            ds.close()
        form, rest = name.split("<")
        f = int(rest.split(",")[0])
        seen.add((form, bool(f & F_MEDIA), bool(f & F_GBVH)))
    assert {("k_fast_sort", False, False), ("k_fast_sort", True, False)} <= seen
    assert {("k_fast", False, False), ("k_fast", False, True), ("k_fast", True, True)} <= seen
