#!/usr/bin/env python3
"""What rtw_scene_query reports (kernel, kernel_fast, bvh_lds_nodes,
shade_lds_bytes) for every scene of tests/golden/scene_*.json but the probe
scenes (scene_probe_*.json: their kernels are listed, with the renders that
drive them, in profiles/probe_reference/kernels_by_case.txt) and the scene of
coincident primitives (scene_ties.json: profiles/ties/kernels_by_case.txt), flat and with
BVHs, under the environments that steer kernel selection: {}, RTW_MODE=wavefront
and wavefront + RTW_SPLIT=1 in this process (read at every call), RTW_SORT=0
and RTW_SORT=1 in one child process each (read once).  Prints one JSON
document: tests/golden/scene_query_gfx950.json is its output on an MI355X
(tests/test_gpu_scene_query.py)."""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FIELDS = ("kernel", "kernel_fast", "bvh_lds_nodes", "shade_lds_bytes")
IN_PROCESS = {"default": {}, "wavefront": {"RTW_MODE": "wavefront"},
              "wavefront_split": {"RTW_MODE": "wavefront", "RTW_SPLIT": "1"}}
CHILDREN = {"sort0": {"RTW_SORT": "0"}, "sort1": {"RTW_SORT": "1"}}
KNOBS = ("RTW_MODE", "RTW_SPLIT", "RTW_SORT", "RTW_FAST_SORT", "RTW_LDS_NODES")


def query_all():
    """{scene/flat|bvh: {field: value}} under the current environment."""
    from raytracingweekend_amd import render
    out = {}
    for p in sorted((ROOT / "tests" / "golden").glob("scene_*.json")):
        name, aspect = p.stem[len("scene_"):], json.loads(p.read_text()).get("aspect")
        if name.startswith("probe_") or name == "ties":  # (younger than the recording; profiles/ties/ lists its kernels)
            continue
        for bvh in (False, True) if aspect else ():  # (this script's own output is no scene dump)
            ds = render.DeviceScene(render.SceneDesc(name, aspect, use_bvh=bvh))
            try:
                info = ds.query()
            finally:
                ds.close()
            out[f"{name}/{'bvh' if bvh else 'flat'}"] = {k: info[k] for k in FIELDS}
    return out


def record():
    rec, saved = {}, {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        for key, env in IN_PROCESS.items():
            os.environ.update(env)
            rec[key] = query_all()
            for k in env:
                del os.environ[k]
        for key, env in CHILDREN.items():  # one after another: one process on the GPU at a time
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child"], env={**os.environ, **env},
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError(f"child {key} failed ({r.returncode}): {r.stderr[-2000:]}")
            rec[key] = json.loads(r.stdout)
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return rec


if __name__ == "__main__":
    rec = query_all() if "--child" in sys.argv else record()
    print(json.dumps(rec, sort_keys=True).replace("}, ", "},\n"))  # one line per scene
