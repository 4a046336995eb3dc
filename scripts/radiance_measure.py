"""Rates of the radiance query (include/rtw_radiance.h) on one GPU, for
profiles/radiance_query/results.txt: rtw_trace_radiance on a render's own camera
rays (rtw_camera_rays and the states it leaves, one sample per ray) next to
rtw_render_accumulate on the same samples, in the same process -- the
persistent ray row the scene selects by default, and the wavefront form
(RTW_MODE=wavefront, read at every call) the same scene would take without the
row.  Device events (ms_total), device buffers, one warm-up round, then the
median and the range of ROUNDS rounds that alternate the three calls.

  python scripts/radiance_measure.py [rounds]
"""
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from raytracingweekend_amd import render  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
DEPTH = 50
CASES = [("cornell_box", False, 800, 800, 4), ("random_balls", False, 1200, 800, 4), ("random_balls", True, 1200, 800, 4),
         ("book2_final", True, 800, 800, 2)]


def stat(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    import torch
    os.environ.pop("RTW_MODE", None)
    print(f"build {render.build_id()}  rounds {ROUNDS}  depth {DEPTH}  (ms: median [min, max]; Msamples/s from the median)")
    for scene, bvh, nx, ny, spp in CASES:
        ds = render.DeviceScene(render.SceneDesc(scene, nx / ny, use_bvh=bvh))
        try:
            rays, rng = ds.camera_rays(nx, ny, spp, 0, device=True)
            n = rays.shape[0]
            acc = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda")
            sums = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
            names = {"render": ds.query()["kernel"], "rays": ds.query_radiance()}
            os.environ["RTW_MODE"] = "wavefront"
            names["rays_wavefront"] = ds.query_radiance()
            del os.environ["RTW_MODE"]
            ms = {k: [] for k in names}
            seg = {}
            for r in range(ROUNDS + 1):
                _, st = ds.render_accumulate(nx, ny, spp, DEPTH, 0, accum=acc)
                t = {"render": st["ms_total"]}
                seg["render"] = st["segments"]
                ds.trace_radiance(rays, 1, DEPTH, rng=rng, out=sums)
                t["rays"], seg["rays"] = ds.last_query_stats["ms_total"], ds.last_query_stats["segments"]
                os.environ["RTW_MODE"] = "wavefront"
                ds.trace_radiance(rays, 1, DEPTH, rng=rng, out=sums)
                del os.environ["RTW_MODE"]
                t["rays_wavefront"] = ds.last_query_stats["ms_total"]
                seg["rays_wavefront"] = ds.last_query_stats["segments"]
                if r:  # (round 0 warms up)
                    for k, v in t.items():
                        ms[k].append(v)
            assert seg["render"] == seg["rays"] == seg["rays_wavefront"], seg
            print(f"{scene} {'bvh' if bvh else 'flat'} {nx}x{ny}x{spp}: {n} samples, {seg['render']} segments each way")
            base = stat(ms["render"])[0]
            for k in ms:
                med, lo, hi = stat(ms[k])
                print(f"  {k:15s} {med:9.3f} ms [{lo:.3f}, {hi:.3f}]  {n / med / 1e3:8.1f} Msamples/s  "
                      f"{base / med:5.3f} of the render  {names[k]}")
        finally:
            ds.close()


if __name__ == "__main__":
    main()
