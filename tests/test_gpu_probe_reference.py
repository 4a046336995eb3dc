"""The fp64 GPU mode on the probe scenes (probe_scene, csrc/host/scenes.cpp)
against the reference's own renders of them, and every execution form of the
fp64 mode on them.

tests/golden/render_probe_*.npy were rendered by the reference's classes on
the probe scenes composed from its headers (oracle/ref_harness.cpp
probe_ref_scene; cases in tests/golden/renders.json, recorded by
oracle/make_golden.py): one render per kind at 32x24x4, depth 50, and the
narrow shutter, a depth cut-off inside the media, a deeper glass render,
Normal mode on the movers and more lens draws per pixel.  Only tests/golden/
is read here.

* Against the reference: per case, flat and with BVHs, the finalized canvas is
  within the project's tolerance of the reference's (1e-4 per channel, as
  tests/test_gpu_parity.py), with the reference's number of world traversals.
* Execution forms: per kind, flat and with BVHs, the persistent kernel,
  the fused wavefront kernel and the split pair are bit-identical with equal
  traversal counts; the RTW_SORT=0/1 children run on the flat scene, where
  k_persist_sort is the default, and for the medium also under BVHs.
  `pytest -s` prints the kernels recorded in
  profiles/probe_reference/kernels_by_case.txt.
"""
import json
from pathlib import Path

import numpy as np
import pytest

from execution_forms import execution_forms_agree
from oracle_lib import case_camera, finalize_np
from raytracingweekend_amd import _abi

pytestmark = pytest.mark.gpu

TOL = 1e-4  # the project's written tolerance (tests/test_gpu_parity.py)

GOLD = Path(__file__).resolve().parent / "golden"
CASES = [c for c in json.loads((GOLD / "renders.json").read_text()) if c["scene"].startswith("probe_")]
KINDS = ["rect_light", "sphere_light", "far_sphere_light", "default_light", "glass", "metal", "medium", "motion",
         "textures"]
FORMS_SIZE = (32, 24, 4, 50)


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


def test_every_kind_has_a_reference_render():
    assert {c["scene"] for c in CASES} == {f"probe_{k}" for k in KINDS}
    assert sum(1 for c in CASES if "shutter" in c) == 2
    assert sum(1 for c in CASES if c.get("render_type") == "normal") == 2
    seeds = [c["seed"] for c in CASES]
    assert len(set(seeds)) == len(seeds)


@pytest.mark.parametrize("bvh", [False, True], ids=["flat", "bvh"])
@pytest.mark.parametrize("case", CASES, ids=[c["case"] for c in CASES])
def test_canvas_matches_the_reference_render(gpu, case, bvh):
    nx, ny, spp = case["nx"], case["ny"], case["spp"]
    sd = gpu.SceneDesc(case["scene"], nx / ny, use_bvh=bvh)
    if case.get("render_type", "shaded") == "normal":
        sd.desc.render_type = _abi.RTW_RENDER_NORMAL
    ds = gpu.DeviceScene(sd)
    try:
        acc, st = ds.render_accumulate(nx, ny, spp, case["max_depth"], seed=case["seed"],
                                       camera=case_camera(sd, case))
        kernel = ds.query()["kernel"]
    finally:
        ds.close()
    gold = np.load(GOLD / f"render_{case['case']}.npy")
    print(f"KERNELS reference {case['case']} bvh={bvh}: {kernel}")
    assert np.all(np.isfinite(gold)), "the reference's render is finite"
    assert np.all(np.isfinite(acc))
    assert st["samples"] == nx * ny * spp
    assert st["segments"] == case["segments"], "device-counted traversals differ from the reference's"
    d = np.abs(finalize_np(acc, spp) - finalize_np(gold, spp))
    assert d.max() <= TOL, f"max per-channel diff {d.max()} at {np.argmax(d)}"


@pytest.mark.parametrize("bvh", [False, True], ids=["flat", "bvh"])
@pytest.mark.parametrize("kind", KINDS)
def test_execution_forms_agree_on_the_probe(gpu, monkeypatch, kind, bvh):
    """k_persist_sort is the default of a scene without BVH features
    (rtw_select.h persist_choice), which every flat probe is: the RTW_SORT
    pair runs there, and under BVHs too for the medium."""
    kernels = execution_forms_agree(gpu, monkeypatch, f"probe_{kind}", bvh, size=FORMS_SIZE,
                                    sort_pair=not bvh or kind == "medium")
    assert kernels[0].startswith("k_persist_sort<" if not bvh else "k_persist<")


@pytest.mark.parametrize("bvh", [False, True], ids=["flat", "bvh"])
def test_execution_forms_agree_on_the_movers_in_normal_mode(gpu, monkeypatch, bvh):
    execution_forms_agree(gpu, monkeypatch, "probe_motion", bvh, normal=True, size=FORMS_SIZE, sort_pair=not bvh)
