"""Helper of the GPU tests that compare the execution forms of the fp64 mode
(test_gpu_parity.py on the built-in scenes, test_gpu_probe_reference.py on the
probe scenes): the persistent kernel with material regrouping
(k_persist_sort) and without it (k_persist) -- RTW_SORT=1/0, read once per
process, so run in child processes -- the wavefront's fused
traversal+shading kernel (k_segment; RTW_MODE=wavefront) and its split pair
(k_intersect, k_shade; + RTW_SPLIT=1) run the same arithmetic in the same
order per sample: bit-identical accumulators and segment counts.  No tests
here."""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

from raytracingweekend_amd import _abi

ROOT = Path(__file__).resolve().parents[1]


def render_in_child(env, scene, nx, ny, spp, depth, seed, bvh, normal=False):
    """Render in a fresh process with extra environment (for switches the
    library reads once per process).  Returns (accumulator, segments)."""
    with tempfile.TemporaryDirectory() as td:
        out = Path(td) / "acc.npy"
        code = (f"import sys; sys.path.insert(0, {str(ROOT)!r}); import numpy as np; "
                f"from raytracingweekend_amd import render as r, _abi; "
                f"sd = r.SceneDesc({scene!r}, {nx}/{ny}, use_bvh={bvh}); "
                f"sd.desc.render_type = _abi.RTW_RENDER_NORMAL if {normal} else sd.desc.render_type; "
                f"ds = r.DeviceScene(sd); "
                f"a, st = ds.render_accumulate({nx}, {ny}, {spp}, {depth}, seed={seed}); ds.close(); "
                f"np.save({str(out)!r}, a); print('SEGMENTS', st['segments'])")
        r = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, check=True, timeout=300,
                           capture_output=True, text=True)
        return np.load(out), int(r.stdout.split("SEGMENTS")[-1].split()[0])


def execution_forms_agree(gpu, monkeypatch, scene, bvh, normal=False, size=(40, 30, 4, 50), sort_pair=True):
    """The in-process forms (persistent, wavefront, split wavefront) and, with
    sort_pair, the RTW_SORT=0/1 children render `scene` bit-identically with
    equal segment counts.  Returns the three in-process kernel names."""
    nx, ny, spp, depth = size
    sd = gpu.SceneDesc(scene, nx / ny, use_bvh=bvh)
    if normal:
        sd.desc.render_type = _abi.RTW_RENDER_NORMAL
    ds = gpu.DeviceScene(sd)
    try:
        a, sa = ds.render_accumulate(nx, ny, spp, depth, seed=5)
        kernels = [ds.query()["kernel"]]
        monkeypatch.setenv("RTW_MODE", "wavefront")
        b, sb = ds.render_accumulate(nx, ny, spp, depth, seed=5)
        kernels.append(ds.query()["kernel"])
        monkeypatch.setenv("RTW_SPLIT", "1")
        c, sc = ds.render_accumulate(nx, ny, spp, depth, seed=5)
        kernels.append(ds.query()["kernel"])
    finally:
        ds.close()
    print(f"KERNELS forms {scene} bvh={bvh} normal={normal}: {kernels}")
    assert kernels[0].startswith("k_persist") and kernels[1].startswith(("k_segment<", "k_intersect<"))
    assert kernels[2].startswith("k_intersect<")
    assert sa["segments"] == sb["segments"] == sc["segments"]
    if normal:
        assert sa["segments"] == nx * ny * spp
    assert np.array_equal(a, b) and np.array_equal(a, c)
    for sort in ("0", "1") if sort_pair else ():
        d, sd_ = render_in_child({"RTW_SORT": sort}, scene, nx, ny, spp, depth, 5, bvh, normal)
        assert np.array_equal(a, d), f"RTW_SORT={sort}"
        assert sd_ == sa["segments"], f"RTW_SORT={sort}"
    return kernels
