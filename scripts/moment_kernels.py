#!/usr/bin/env python3
"""The estimator and finalize kernels, 20 calls each at 800x800 on device
tensors: the uniform estimate, the estimate with counts and the three canvases.
Run it under `rocprofv3 --kernel-trace --stats -- python scripts/moment_kernels.py`
once per library (RTW_LIBRARY) and compare the kernels' rows
(profiles/moment_stats/results.txt)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

if __name__ == "__main__":
    import torch
    from raytracingweekend_amd import render

    nx = ny = 800
    rng = np.random.default_rng(1)
    counts = rng.integers(2, 64, nx * ny).astype(np.int32)
    s1 = rng.random(nx * ny * 3) * np.repeat(counts, 3)
    s2 = s1 * s1 / np.repeat(counts, 3) * (1.0 + rng.random(nx * ny * 3))
    ds = render.DeviceScene(render.SceneDesc("cornell_box", 1.0))
    try:
        t1, t2, tc = (torch.from_numpy(a).to("cuda:0") for a in (s1, s2, counts))
        for _ in range(20):
            ds.noise_estimate(t1, t2, nx, ny, 16)
            ds.noise_estimate_counts(t1, t2, tc, nx, ny)
            ds.finalize_device(t1, nx, ny, 16)
            ds.finalize_counts(t1, tc, nx, ny)
            ds.finalize_mean(t1, nx, ny)
    finally:
        ds.close()
    print("moment_kernels: 20 calls of each done")
