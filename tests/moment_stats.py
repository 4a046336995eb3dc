"""What the public moment-statistics entry points return on fixed inputs, as
hashes and hex floats: the noise estimate with one n and with counts, the
active list, the three canvases and denoise(iterations=0).  Shared by
scripts/record_moment_stats.py, which wrote tests/golden/moment_stats_parent.json
from the library before the per-pixel arithmetic moved into csrc/host/moments.h,
and tests/test_moment_stats.py, which demands those bits of the library now."""
import hashlib
import json
from pathlib import Path

import numpy as np

from test_adaptive import MAX_COUNT, SIZES, moments, rel_np
from test_noise import FLOOR

GOLDEN = Path(__file__).resolve().parent / "golden" / "moment_stats_parent.json"
# mixed: the generator's counts (0, 1, 2 and the maximum among them), n = 7 where one n is asked for
MODES = {"mixed": 7, "n2": 2, "n7": 7}


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def summary_hex(s: dict) -> dict:
    return {k: (v.hex() if isinstance(v, float) else int(v)) for k, v in s.items()}


def case(render, nx: int, ny: int, mode: str, ds=None) -> dict:
    """One case through `render`'s host functions, or (ds: a DeviceScene) with
    torch tensors through the device entry points."""
    s1, s2, counts = moments(nx, ny)
    n = MODES[mode]
    if mode != "mixed":
        counts = np.full(nx * ny, n, dtype=np.uint32)
    rel, _, fin = rel_np(s1, s2, counts)
    judged = fin & (counts >= 2) & (counts < MAX_COUNT)
    half = float(np.median(rel[judged])) if judged.any() else 0.02
    feat = np.zeros(nx * ny * 8)
    if ds is None:
        a1, a2, ac, af, api, host = s1, s2, counts, feat, render, np.asarray
    else:
        import torch
        a1, a2, af = (torch.from_numpy(x).to(f"cuda:{ds.device}") for x in (s1, s2, feat))
        ac = torch.from_numpy(counts.astype(np.int32)).to(a1.device)
        api, host = ds, lambda t: t.cpu().numpy()
    out = {"inputs": sha(s1) + sha(s2) + sha(counts), "target_median": half.hex()}
    se, summ = api.noise_estimate(a1, a2, nx, ny, n, FLOOR)
    out["stderr_n"], out["summary_n"] = sha(host(se)), summary_hex(summ)
    se, summ = api.noise_estimate_counts(a1, a2, ac, nx, ny, FLOOR)
    out["stderr_counts"], out["summary_counts"] = sha(host(se)), summary_hex(summ)
    for name, target in (("0", 0.0), ("1e9", 1e9), ("median", half)):
        act = api.select_active(a1, a2, ac, nx, ny, target_rel=target, max_count=MAX_COUNT, floor=FLOOR)
        out[f"active_{name}"] = sha(host(act).astype(np.uint32))
    for key, kw in (("n", {"n": n}), ("counts", {"counts": ac})):
        mean, var = api.denoise(a1, a2, af, nx, ny, feature_spp=1, want_variance=True, iterations=0, **kw)
        out[f"denoise_{key}_mean"], out[f"denoise_{key}_var"] = sha(host(mean)), sha(host(var))
    out["canvas_n"] = sha(render.finalize(s1, nx, ny, n) if ds is None else host(ds.finalize_device(a1, nx, ny, n)))
    out["canvas_counts"] = sha(host(api.finalize_counts(a1, ac, nx, ny)))
    out["canvas_mean"] = sha(host(api.finalize_mean(mean, nx, ny)))
    return out


def record(render, device: bool) -> dict:
    """{"<nx>x<ny>/<mode>": case} of every size and mode, host or device."""
    ds = render.DeviceScene(render.SceneDesc("cornell_box", 1.0)) if device else None
    try:
        return {f"{nx}x{ny}/{mode}": case(render, nx, ny, mode, ds) for nx, ny in SIZES for mode in MODES}
    finally:
        if ds is not None:
            ds.close()


def golden(half: str) -> dict:
    return json.loads(GOLDEN.read_text())[half]
