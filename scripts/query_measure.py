"""Rates of the ray queries (include/rtw_query.h) on one GPU, for
profiles/ray_query/results.txt: rtw_trace_closest on a render's camera rays next
to k_features on the same camera samples, and rtw_trace_occluded against
rtw_trace_closest on the same rays and on a batch of shadow-like rays (from each
first hit towards the scene's light, or towards a fixed sun where it has none).
Device events (ms_total), one warm-up call each, the median and the range of
ROUNDS calls, the variants alternating in one process.

  python scripts/query_measure.py [rounds]
"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from raytracingweekend_amd import render  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
CASES = [("cornell_box", False, 800, 800, 4), ("random_balls", False, 1200, 800, 4), ("random_balls", True, 1200, 800, 4),
         ("book2_final", True, 800, 800, 2)]


def light_target(desc):
    """Centre of the scene's first light primitive, or None."""
    if desc.n_lights == 0 or desc.lights[0].kind == 0:
        return None
    p = desc.prims[desc.lights[0].prim]
    v = p.p[:]
    if p.type in (0, 1):
        return np.array(v[:3])
    a, b, k = {2: (0, 1, 2), 3: (0, 2, 1), 4: (1, 2, 0)}[p.type]
    c = np.zeros(3)
    c[a], c[b], c[k] = 0.5 * (v[0] + v[1]), 0.5 * (v[2] + v[3]), v[4]
    return c


def stat(ms):
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    import torch
    print(f"build {render.build_id()}  rounds {ROUNDS}  (ms: median [min, max]; Mrays/s from the median)")
    for scene, bvh, nx, ny, spp in CASES:
        sd = render.SceneDesc(scene, nx / ny, use_bvh=bvh)
        ds = render.DeviceScene(sd)
        try:
            names = ds.query_trace()
            media = names[0] in ("k_query<1>", "k_query<5>")
            rays, rng = ds.camera_rays(nx, ny, spp, 0, device=True)
            n = rays.shape[0]
            feat = torch.zeros(nx * ny * 8, dtype=torch.float64, device="cuda")
            g = lambda: rng.clone() if media else None
            # shadow-like rays from the first hits
            h = ds.trace_rays(rays, g())
            hit = h["prim"] != -1
            o = (h["p"] + 1e-6 * h["n"])[hit]
            tgt = light_target(sd.desc)
            shadow = torch.empty((o.shape[0], 8), dtype=torch.float64, device="cuda")
            shadow[:, :3] = o
            if tgt is None:
                shadow[:, 3:6] = torch.tensor([0.3, 1.0, 0.2], dtype=torch.float64, device="cuda")
                shadow[:, 7] = float("inf")
            else:
                shadow[:, 3:6] = torch.tensor(tgt, device="cuda") - o
                shadow[:, 7] = 0.999
            shadow[:, 6] = rays[hit, 6]
            shadow_rng = rng[hit].contiguous()
            gs = lambda: shadow_rng.clone() if media else None
            ms = {k: [] for k in ("features", "closest", "occluded", "closest_shadow", "occluded_shadow")}
            for r in range(ROUNDS + 1):
                _, st = ds.render_features(nx, ny, spp, 0, features=feat)
                t = {"features": st["ms_total"]}
                ds.trace_rays(rays, g())
                t["closest"] = ds.last_query_stats["ms_total"]
                ds.trace_rays(rays, g(), occluded=True)
                t["occluded"] = ds.last_query_stats["ms_total"]
                ds.trace_rays(shadow, gs())
                t["closest_shadow"] = ds.last_query_stats["ms_total"]
                occ = ds.trace_rays(shadow, gs(), occluded=True)
                t["occluded_shadow"] = ds.last_query_stats["ms_total"]
                if r:  # (round 0 warms up)
                    for k, v in t.items():
                        ms[k].append(v)
            print(f"{scene} {'bvh' if bvh else 'flat'} {nx}x{ny}x{spp}: {n} camera rays ({int(hit.sum())} hit), "
                  f"{shadow.shape[0]} shadow rays ({int(occ.sum())} occluded, "
                  f"{'towards the light' if tgt is not None else 'towards a sun'})  {names[0]} {names[1]}")
            for k in ms:
                med, lo, hi = stat(ms[k])
                cnt = shadow.shape[0] if k.endswith("shadow") else n
                print(f"  {k:16s} {med:9.3f} ms [{lo:.3f}, {hi:.3f}]  {cnt / med / 1e3:9.1f} M/s")
        finally:
            ds.close()


if __name__ == "__main__":
    main()
