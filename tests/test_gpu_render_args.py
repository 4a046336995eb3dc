"""rtw_render_accumulate's refusals through the C ABI (the Python wrapper
would refuse some of them first): each returns RTW_ERR_INVALID with its text
and touches nothing -- afterwards the same handle renders 8 x 8 x 4 spp bit
for bit as a fresh handle does, and a call whose sample range is empty leaves
the accumulator as it was and reports samples = 0.  The smallest built-in
list scene (`dielectric`) at 8 x 8, depth 5; the shutter refusal needs moving
spheres under a BVH (`random_balls` with use_bvh).  The texts are those of
tests/golden/render_plan_parent.json (tests/test_render_plan.py)."""
import copy
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from raytracingweekend_amd import _abi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "render_plan_parent.json"
NX = NY = 8
DEPTH = 5
# the golden's case -> the parameters that differ from an 8 x 8 x 8 spp call
REFUSALS = {
    "nx_zero": dict(nx=0),
    "spp_zero": dict(spp=0),
    "begin_past_spp": dict(spp_begin=9),
    "count_negative": dict(spp_count=-1),
    "range_past_spp": dict(spp_begin=5, spp_count=4),
    "precision_7": dict(precision=7),
    "row_begin_minus1": dict(row_begin=-1),
    "row_begin_ny": dict(row_begin=NY),
    "image_65536": dict(nx=65536, ny=65536, spp=1),
    "image_46341": dict(nx=46341, ny=46341, spp=1),
}


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


def params(**kw):
    p = dict(nx=NX, ny=NY, spp=8, max_depth=DEPTH, seed=11, spp_begin=0, spp_count=0, row_begin=0, row_step=1,
             accum_on_device=0, collect_kernel_times=0, wavefront_paths=0, precision=0)
    p.update(kw)
    return _abi.rtw_render_params(**p)


def call(ds, cam, prm, accum, accum_sq=None):
    """(code, last error text, stats) of one call through the C ABI."""
    L, st = _abi.lib(), _abi.rtw_stats()
    ptr = accum.ctypes.data_as(C.c_void_p)
    if accum_sq is None:
        rc = L.rtw_render_accumulate(ds.handle, C.byref(cam), C.byref(prm), ptr, C.byref(st))
    else:
        rc = L.rtw_render_accumulate_moments(ds.handle, C.byref(cam), C.byref(prm), ptr, accum_sq, C.byref(st))
    return rc, (L.rtw_last_error() or b"").decode(), st


def test_refusals_leave_the_handle_as_it_was(gpu):
    want = json.loads(GOLDEN.read_text())["cases"]
    sd = gpu.SceneDesc("dielectric", NX / NY)
    ds = gpu.DeviceScene(sd)
    fresh = gpu.DeviceScene(sd)
    try:
        cam = sd.camera
        canary = np.full(NX * NY * 3, 0.25)
        for name, kw in REFUSALS.items():
            rc, text, _ = call(ds, cam, params(**kw), canary)
            assert (rc, text) == (want[name]["rc"], want[name]["error"]) and rc == -1, name
        # overlapping moment buffers (the second starts one double into the first)
        both = np.full(NX * NY * 3 + 1, 0.25)
        rc, text, _ = call(ds, cam, params(), both, C.c_void_p(both.ctypes.data + 8))
        assert (rc, text) == (-1, want["moments_overlap"]["error"])
        assert np.all(canary == 0.25) and np.all(both == 0.25)

        # the handle renders as a fresh one does
        got, ref = np.zeros(NX * NY * 3), np.zeros(NX * NY * 3)
        rc, text, st = call(ds, cam, params(spp=4), got)
        assert rc == 0 and st.samples == NX * NY * 4, text
        rc, text, _ = call(fresh, cam, params(spp=4), ref)
        assert rc == 0, text
        assert np.array_equal(got, ref) and np.all(np.isfinite(got)) and got.any()

        # no samples: the accumulator is untouched
        before = got.copy()
        rc, text, st = call(ds, cam, params(spp=4, spp_begin=4), got)
        assert rc == 0 and st.samples == 0 and st.segments == 0 and st.launches_intersect == 0, text
        assert np.array_equal(got, before)
        # ... and depth 0: every sample adds zero
        rc, text, st = call(ds, cam, params(spp=4, max_depth=0), got)
        assert rc == 0 and st.samples == NX * NY * 4 and st.segments == 0, text
        assert np.array_equal(got, before)
    finally:
        ds.close()
        fresh.close()


def test_shutter_refusal_text(gpu):
    want = json.loads(GOLDEN.read_text())["cases"]["shutter_outside"]
    sd = gpu.SceneDesc("random_balls", NX / NY, use_bvh=True)
    ds = gpu.DeviceScene(sd)
    try:
        cam = copy.copy(sd.camera)
        cam.time1 = cam.time1 + 1.0
        canary = np.full(NX * NY * 3, 0.25)
        rc, text, _ = call(ds, cam, params(), canary)
        assert (rc, text) == (want["rc"], want["error"]) and rc == -1
        assert np.all(canary == 0.25)
    finally:
        ds.close()
