"""Measurements of adaptive sampling (profiles/adaptive/results.txt)
on one MI355X.  Not a test: prints figures.

  python scripts/adaptive_measure.py cost      # the indirection: identity list vs render_moments
  python scripts/adaptive_measure.py gain      # render_adaptive vs render_to_noise at one target per scene

cost: Cornell 800x800 and random_balls 1200x800 with BVHs, 128 spp, depth 50,
fp64 and fp32, device buffers; the two sides alternate, REPS times each, and
the outputs are compared bit for bit.  gain: Cornell 800x800, random_balls
1200x800 and Book 2 800x800 (the last two with BVHs), depth 50; the target is
half the mean_rel of a 64-sample render, three quarters of it for Book 2 (the
uniform loop reaches each at 512 spp; profiles/adaptive/results.txt 2b has the
Book 2 run with half); both loops start at 16 samples and double, max_spp 1024; the sides
alternate, GAIN_REPS timed pairs after a warm-up pair, with device buffers and
with host buffers; the canvases are compared with a uniform render of
4 x max_spp samples of another seed.
"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1]))
from raytracingweekend_amd import render  # noqa: E402

DEPTH, FLOOR, REPS, GAIN_REPS = 50, 1e-2, 5, 3
DEV = "cuda:0"


def spread(xs):
    return f"{np.mean(xs):9.3f} (min {min(xs):.3f} max {max(xs):.3f})"


def cost():
    for scene, bvh, nx, ny in (("cornell_box", False, 800, 800), ("random_balls", True, 1200, 800)):
        ds = render.DeviceScene(render.SceneDesc(scene, nx / ny, use_bvh=bvh))
        ident = torch.arange(nx * ny, dtype=torch.int32, device=DEV)
        for precision in ("fp64", "fp32"):
            t = {"moments": ([], []), "active": ([], [])}
            out = {}
            for rep in range(REPS + 1):  # (the first pair warms up)
                for side in ("moments", "active"):
                    a = torch.zeros(nx * ny * 3, dtype=torch.float64, device=DEV)
                    q = torch.zeros_like(a)
                    if side == "moments":
                        _, _, st = ds.render_moments(nx, ny, 128, DEPTH, 1, accum=a, accum_sq=q, precision=precision,
                                                     collect_kernel_times=True)
                    else:
                        st = ds.render_active(nx, ny, 128, DEPTH, 1, active=ident, accum=a, accum_sq=q,
                                              precision=precision, collect_kernel_times=True)
                    if rep:
                        t[side][0].append(st["ms_intersect"])
                        t[side][1].append(st["ms_total"])
                    out[side] = (a, q)
            same = all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(out["moments"], out["active"]))
            names = ds.query()["kernel" if precision == "fp64" else "kernel_fast"], ds.query_active(precision)
            print(f"cost {scene}{'/bvh' if bvh else ''} {nx}x{ny}x128 {precision}: bit-equal {same}; {names[0]} vs {names[1]}")
            for side in ("moments", "active"):
                print(f"    {side:8s} ms_intersect {spread(t[side][0])}   ms_total {spread(t[side][1])}")
            di = np.mean(t["active"][0]) / np.mean(t["moments"][0]) - 1
            dt = np.mean(t["active"][1]) / np.mean(t["moments"][1]) - 1
            sp = [100 * (max(t[side][k]) / min(t[side][k]) - 1) for k in (0, 1) for side in ("moments", "active")]
            print(f"    active / moments - 1: ms_intersect {100 * di:+.2f} % (spread of the repeats: moments {sp[0]:.2f} %, "
                  f"active {sp[1]:.2f} %)   ms_total {100 * dt:+.2f} % (moments {sp[2]:.2f} %, active {sp[3]:.2f} %)")
        ds.close()


def gain():
    max_spp, min_spp = 1024, 16
    # (Book 2's heavy tails: its mean_rel falls more slowly than 1 / sqrt(n) -- 0.351 at 64 samples, 0.191 at
    # 1 024, profiles/adaptive/results.txt 2b -- so half the 64-sample figure is out of the uniform loop's reach;
    # three quarters is not)
    for scene, bvh, nx, ny, part in (("cornell_box", False, 800, 800, 0.5), ("random_balls", True, 1200, 800, 0.5),
                                     ("book2_final", True, 800, 800, 0.75)):
        ds = render.DeviceScene(render.SceneDesc(scene, nx / ny, use_bvh=bvh))
        a, q, _ = ds.render_moments(nx, ny, max_spp, DEPTH, 1, spp_begin=0, spp_count=64,
                                    accum=torch.zeros(nx * ny * 3, dtype=torch.float64, device=DEV))
        target = part * ds.noise_estimate(a, q, nx, ny, 64, FLOOR, want_stderr=False)[1]["mean_rel"]
        ref, _ = ds.render_accumulate(nx, ny, 4 * max_spp, DEPTH, 2,
                                      accum=torch.zeros(nx * ny * 3, dtype=torch.float64, device=DEV))
        ref = ds.finalize_device(ref, nx, ny, 4 * max_spp).cpu().numpy()
        print(f"gain {scene}{'/bvh' if bvh else ''} {nx}x{ny} depth {DEPTH}: target_rel {target:.5f}, min_spp {min_spp}, "
              f"max_spp {max_spp}, doubling; reference {4 * max_spp} spp, seed 2")
        for dev_buf in (True, False):
            wall = {"uniform": [], "adaptive": []}
            figures = {}
            for rep in range(GAIN_REPS + 1):  # (the first pair warms up)
                for side in ("uniform", "adaptive"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if side == "uniform":
                        u = render.render_to_noise(ds, nx, ny, max_spp, DEPTH, 1, target=target, first_batch=min_spp,
                                                   floor=FLOOR, device_buffers=dev_buf)
                    else:
                        r = render.render_adaptive(ds, nx, ny, max_spp, DEPTH, 1, target_rel=target, min_spp=min_spp,
                                                   batch=0, floor=FLOOR, device_buffers=dev_buf)
                    torch.cuda.synchronize()
                    if rep:
                        wall[side].append(time.perf_counter() - t0)
                if dev_buf:
                    cu = ds.finalize_device(u["accum"], nx, ny, u["spp_done"]).cpu().numpy()
                    ca = ds.finalize_counts(r["accum"], r["counts"], nx, ny).cpu().numpy()
                else:
                    cu = render.finalize(u["accum"], nx, ny, u["spp_done"])
                    ca = render.finalize_counts(r["accum"], r["counts"], nx, ny)
                hu = u["history"][-1]
                fig = (f"    uniform  samples {u['stats']['samples']:>11d} ({u['spp_done']} spp)  rounds {len(u['history'])}  "
                       f"mean_rel {hu[1]:.5f}  max_rel {hu[2]:.5f}  |canvas - ref| {np.abs(cu - ref).mean():.6f}\n"
                       f"    adaptive samples {r['samples']:>11d} ({r['samples'] / (nx * ny):.1f} spp)  rounds {r['rounds']}  "
                       f"mean_rel {r['summary']['mean_rel']:.5f}  max_rel {r['summary']['max_rel']:.5f}  "
                       f"|canvas - ref| {np.abs(ca - ref).mean():.6f}  at max_spp {r['pixels_at_max'] / (nx * ny):.4f}  "
                       f"mean canvas, adaptive - uniform {np.mean(ca - cu):+.6f}")
                figures[fig] = figures.get(fig, 0) + 1
            print(f"  {'device' if dev_buf else 'host'} buffers, {GAIN_REPS} timed pairs after one warm-up pair:")
            for fig, k in figures.items():  # (the same seed: every repeat gives the same figures)
                print(f"   in {k} of {GAIN_REPS + 1} pairs:\n{fig}")
            for side in ("uniform", "adaptive"):
                print(f"    {side:8s} wall s {spread(wall[side])}")
            print(f"    adaptive / uniform - 1: samples {100 * (r['samples'] / u['stats']['samples'] - 1):+.1f} % (no spread: "
                  f"deterministic)   wall {100 * (np.mean(wall['adaptive']) / np.mean(wall['uniform']) - 1):+.1f} % "
                  f"(spread of the repeats: uniform {100 * (max(wall['uniform']) / min(wall['uniform']) - 1):.1f} %, "
                  f"adaptive {100 * (max(wall['adaptive']) / min(wall['adaptive']) - 1):.1f} %)")
        ds.close()


if __name__ == "__main__":
    {"cost": cost, "gain": gain}[sys.argv[1]]()
