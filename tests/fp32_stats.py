"""The statistic that compares the fp32 fast mode with the reference's
estimator (tests/test_gpu_fp32.py explains it; test_gpu_bvh_forms.py applies
it in Normal mode): 8x8-pixel block means of three fast-mode renders and of
three fp64 renders with other seeds, both against the oracle's render, and the
spread and bias inequalities between them.  No tests here."""
import numpy as np

FAST_SEEDS = (0, 1, 2)   # fp32 renders
OTHER_SEEDS = (1, 2, 3)  # fp64 renders with independent noise
REF_SEED = 0             # the oracle's render


def blocks(acc, nx, ny, spp, b=8):
    img = (acc / spp).reshape(ny, nx, 3)
    return img.reshape(ny // b, b, nx // b, b, 3).mean(axis=(1, 3)).reshape(-1, 3)


def render_sets(ds, nx, ny, spp, depth):
    """([(accum, stats)] of the fast-mode seeds, the same of the other fp64
    seeds) from a DeviceScene."""
    fast = [ds.render_accumulate(nx, ny, spp, depth, seed=k, precision="fp32") for k in FAST_SEEDS]
    other = [ds.render_accumulate(nx, ny, spp, depth, seed=k) for k in OTHER_SEEDS]
    return fast, other


def assert_statistically_the_reference(fast, other, ref, nx, ny, spp):
    """fast, other: accumulators (per-pixel sums over spp samples) of the
    fp32 renders and of the fp64 renders with other seeds; ref: the oracle's.
    With d_b = fast block mean - oracle's and e_b = other-seed fp64 block
    mean - oracle's:
      spread:  mean(d_b^2) < 2 mean(e_b^2)  (F-ratio over >= 96 block
               differences; the 99.9th percentile of F(96, 96) is about 1.9)
      bias:    |mean(d_b)| < 4 sqrt(mean(e_b^2) / B) + 1e-3 |image mean|"""
    rb = blocks(ref, nx, ny, spp)
    d = np.concatenate([blocks(acc, nx, ny, spp) - rb for acc in fast])
    e = np.concatenate([blocks(acc, nx, ny, spp) - rb for acc in other])
    B = d.shape[0]
    assert B >= 96
    spread, base = float((d ** 2).mean()), float((e ** 2).mean())
    assert spread < 2.0 * base, f"block spread {spread:.3e} vs fp64-noise {base:.3e}"
    level = float(np.abs(ref).mean() / spp)
    bias = np.abs(d.mean(axis=0))
    assert np.all(bias < 4 * np.sqrt(base / B) + 1e-3 * level), (bias, np.sqrt(base / B))
    return {"spread": spread, "base": base, "bias": bias.tolist(), "bias_bound": 4 * np.sqrt(base / B) + 1e-3 * level}
