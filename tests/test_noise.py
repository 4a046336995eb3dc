"""Per-pixel noise estimate (include/rtw_noise.h), CPU side: the host
estimator against the same expression in numpy, argument errors, what the
estimate means against a converged oracle render, the render-to-target loop
on a fake scene, and the header / ABI table.  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from raytracingweekend_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "rtw_noise.h"
FLOOR = 1e-2


def noise_np(s1, s2, n, floor=FLOOR):
    """rtw_noise.h's definition, verbatim, on float64 arrays: (stderr map with
    NaN in non-finite pixels, summary dict)."""
    s1 = np.asarray(s1, dtype=np.float64).reshape(-1, 3)
    s2 = np.asarray(s2, dtype=np.float64).reshape(-1, 3)
    dn, dn1 = np.float64(n), np.float64(n - 1)
    with np.errstate(all="ignore"):
        m = s1 / dn
        v = (s2 - s1 * m) / dn1
        v = np.where(v < 0, 0.0, v)
        se = np.sqrt(v / dn)
        rel = ((se[:, 0] + se[:, 1]) + se[:, 2]) / (((m[:, 0] + m[:, 1]) + m[:, 2]) + 3 * np.float64(floor))
    fin = np.isfinite(s1).all(axis=1) & np.isfinite(s2).all(axis=1)
    k = int(fin.sum())
    summary = {"pixels": k, "nonfinite": int((~fin).sum()),
               "mean_rel": float(rel[fin].sum() / k) if k else 0.0,
               "max_rel": float(rel[fin].max()) if k else 0.0,
               "rms_stderr": float(np.sqrt((se[fin] ** 2).sum() / (k * 3.0))) if k else 0.0}
    return np.where(fin[:, None], se, np.nan).reshape(-1), summary


def moments_np(samples):
    """In-order raw moments of per-sample arrays: q = q + x*x, one rounded
    product and one rounded add per sample (numpy does not fuse)."""
    s1 = np.zeros_like(samples[0])
    s2 = np.zeros_like(samples[0])
    for x in samples:
        s1 = s1 + x
        s2 = s2 + x * x
    return s1, s2


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def synthetic(n, nx=5, ny=3, seed=0):
    rng = np.random.default_rng([seed, n])
    x = rng.random((n, nx * ny, 3)) * rng.random((1, nx * ny, 1)) * 4.0
    x[:, 1, :] = 0.25          # a constant pixel: se == 0 exactly
    x[:, 2, :] = 0.7           # constant, inexact: S2 - S1*m cancels below 0 at n = 7 and 64
    x[:, 5, :] = 0.1           # constant, inexact: cancels a few ulps above 0 at n = 7 and 64
    s1, s2 = moments_np(list(x))
    s1[3, 1] = np.nan          # a NaN pixel
    s1[4, 0] = s2[4, 0] = np.inf  # an Inf pixel
    return s1.reshape(-1), s2.reshape(-1)


@pytest.mark.parametrize("n", [2, 7, 64])
def test_host_estimator_matches_numpy(built, n):
    from raytracingweekend_amd import render
    nx, ny = 5, 3
    s1, s2 = synthetic(n)
    se, summ = render.noise_estimate(s1, s2, nx, ny, n, FLOOR)
    want_se, want = noise_np(s1, s2, n)
    assert same_bits(se, want_se), "stderr map differs from the numpy expression"
    assert not se.reshape(-1, 3)[1].any(), "constant pixel must have se == 0"
    assert np.isnan(se.reshape(-1, 3)[3:5]).all() and np.isfinite(se.reshape(-1, 3)[:3]).all()
    assert summ["pixels"] == want["pixels"] == nx * ny - 2
    assert summ["nonfinite"] == want["nonfinite"] == 2
    for k in ("mean_rel", "max_rel", "rms_stderr"):
        assert summ[k] == pytest.approx(want[k], rel=1e-12), k
    # summary only, and map only
    none, summ2 = render.noise_estimate(s1, s2, nx, ny, n, FLOOR, want_stderr=False)
    assert none is None and summ2 == summ
    out = np.empty_like(s1)
    assert _abi.lib().rtw_noise_estimate(s1.ctypes.data_as(C.c_void_p), s2.ctypes.data_as(C.c_void_p), nx, ny, n,
                                         FLOOR, out.ctypes.data_as(C.c_void_p), None) == 0
    assert same_bits(out, se)


def test_negative_variance_is_clamped(built):
    """7 samples all equal to 0.7: S2 - S1*m cancels to -1.3e-15 before the
    clamp (7 samples of 0.1 cancel to +1.4e-17 with in-order sums, so 0.1
    would not reach the clamp); the estimator must give se == 0, not NaN."""
    from raytracingweekend_amd import render
    x = np.full(3, 0.7)
    s1, s2 = moments_np([x] * 7)
    assert (s2 - s1 * (s1 / 7.0) < 0).all(), "the example must exercise the clamp"
    se, summ = render.noise_estimate(s1, s2, 1, 1, 7, FLOOR)
    assert (se == 0).all() and summ["mean_rel"] == 0 and summ["pixels"] == 1


def test_no_finite_pixel_gives_zeros(built):
    from raytracingweekend_amd import render
    s1 = np.full(6, np.nan)
    s2 = np.ones(6)
    se, summ = render.noise_estimate(s1, s2, 2, 1, 4, FLOOR)
    assert np.isnan(se).all()
    assert summ == {"pixels": 0, "nonfinite": 2, "mean_rel": 0.0, "max_rel": 0.0, "rms_stderr": 0.0}


def test_argument_errors(built):
    lib = _abi.lib()
    a, q, se = np.ones(12), np.ones(12), np.ones(12)
    pa, pq, pse = (x.ctypes.data_as(C.c_void_p) for x in (a, q, se))
    out = _abi.rtw_noise_summary()

    def refused(*args, word):
        assert lib.rtw_noise_estimate(*args) == -1
        assert word in lib.rtw_last_error(), lib.rtw_last_error()

    refused(pa, pq, 2, 2, 1, FLOOR, pse, C.byref(out), word=b"n >= 2")
    refused(pa, pq, 2, 2, 4, 0.0, pse, C.byref(out), word=b"floor")
    refused(pa, pq, 2, 2, 4, float("nan"), pse, C.byref(out), word=b"floor")
    refused(None, pq, 2, 2, 4, FLOOR, pse, C.byref(out), word=b"null")
    refused(pa, None, 2, 2, 4, FLOOR, pse, C.byref(out), word=b"null")
    refused(pa, pq, 0, 2, 4, FLOOR, pse, C.byref(out), word=b"image size")
    refused(pa, pa, 2, 2, 4, FLOOR, pse, C.byref(out), word=b"overlap")
    big = np.ones(20)
    refused(big.ctypes.data_as(C.c_void_p), C.c_void_p(big.ctypes.data + 8 * 8), 2, 2, 4, FLOOR, pse, C.byref(out),
            word=b"overlap")
    refused(pa, pq, 2, 2, 4, FLOOR, pq, C.byref(out), word=b"overlap")
    assert (se == 1).all(), "a refused call must not write"
    # the device entry points refuse a null handle before touching any device
    assert lib.rtw_render_accumulate_moments(None, None, None, None, None, None) == -1
    assert b"rtw_render_accumulate_moments" in lib.rtw_last_error()
    assert lib.rtw_noise_estimate_device(None, pa, pq, 2, 2, 4, FLOOR, None, C.byref(out)) == -1
    assert b"null" in lib.rtw_last_error()


@pytest.mark.slow
def test_estimate_covers_the_truth(built):
    """The estimate means what it says: on random_balls 24x16 (depth 50), with
    the moments of 64 samples, |mean - truth| < 3*se in at least 97 % of the
    channels with se > 0, truth being an independent 4096-sample render
    (oracle only).  And mean_rel falls as samples are added."""
    from oracle_lib import oracle_sums
    from raytracingweekend_amd import render
    nx, ny, depth, n = 24, 16, 50, 64
    sd = render.SceneDesc("random_balls", nx / ny)
    samples = [oracle_sums(sd, nx, ny, 4096, depth, seed=9, spp_begin=s, spp_count=1)[0] for s in range(n)]
    # (threads given: the oracle's thread count is sticky across calls, and an
    # earlier test of the session may have left it at 1)
    truth = oracle_sums(sd, nx, ny, 4096, depth, seed=5, threads=min(16, os.cpu_count() or 1))[0] / 4096.0
    s1, s2 = moments_np(samples)
    se, summ = render.noise_estimate(s1, s2, nx, ny, n, FLOOR)
    assert summ["nonfinite"] == 0
    live = se > 0
    inside = np.abs(s1 / n - truth)[live] < 3 * se[live]
    print(f"coverage {inside.mean():.4f} over {live.sum()} channels ({1 - live.mean():.3f} have se == 0)")
    assert inside.mean() >= 0.97
    rels = []
    for k in (8, 16, 32, 64):
        a, q = moments_np(samples[:k])
        rels.append(render.noise_estimate(a, q, nx, ny, k, FLOOR, want_stderr=False)[1]["mean_rel"])
    print("mean_rel at 8/16/32/64:", rels)
    assert all(x > y for x, y in zip(rels, rels[1:])), rels


class FakeScene:
    """Stands in for a DeviceScene in render_to_noise: every channel's samples
    are N(1, sigma^2) keyed by (seed, sample), so sample ranges compose."""
    device = 0

    def __init__(self, sigma):
        self.sigma = sigma
        self.calls = []

    def render_moments(self, nx, ny, spp, max_depth, seed=0, *, spp_begin=0, spp_count=0, accum=None,
                       accum_sq=None, camera=None, precision="fp64"):
        self.calls.append((spp, spp_begin, spp_count))
        for s in range(spp_begin, spp_begin + spp_count):
            x = np.random.default_rng([seed, s]).normal(1.0, self.sigma, nx * ny * 3)
            accum += x
            accum_sq += x * x
        return accum, accum_sq, {"samples": nx * ny * spp_count, "ms_total": 1.0}

    def noise_estimate(self, accum, accum_sq, nx, ny, n, floor=FLOOR, want_stderr=True):
        from raytracingweekend_amd import render
        return render.noise_estimate(accum, accum_sq, nx, ny, n, floor, want_stderr)


def test_render_to_noise_loop(built):
    from raytracingweekend_amd import render
    nx, ny = 16, 8
    # se ~ sigma / sqrt(n), mean 1: mean_rel ~ 0.5 / sqrt(n) / 1.01 = .175 .124 .088 .062 at 8 16 32 64
    ds = FakeScene(0.5)
    r = render.render_to_noise(ds, nx, ny, 256, 50, seed=3, target=0.1, first_batch=8)
    assert ds.calls == [(256, 0, 8), (256, 8, 8), (256, 16, 16)]
    assert r["reached"] and r["spp_done"] == 32
    assert [h[0] for h in r["history"]] == [8, 16, 32]
    assert r["history"][-1][1] <= 0.1 and all(h[1] > 0.1 for h in r["history"][:-1])
    assert all(h[2] >= h[1] for h in r["history"])
    assert r["stats"] == {"samples": nx * ny * 32, "ms_total": 3.0}
    one = FakeScene(0.5)
    a, q, _ = one.render_moments(nx, ny, 256, 50, 3, spp_begin=0, spp_count=32, accum=np.zeros(nx * ny * 3),
                                 accum_sq=np.zeros(nx * ny * 3))
    assert np.allclose(r["accum"], a, rtol=1e-12, atol=1e-12)
    assert np.allclose(r["accum_sq"], q, rtol=1e-12, atol=1e-12)
    # an unreachable target: every batch, the last one cut at max_spp
    ds = FakeScene(0.5)
    r = render.render_to_noise(ds, nx, ny, 50, 50, seed=3, target=1e-6, first_batch=8)
    assert ds.calls == [(50, 0, 8), (50, 8, 8), (50, 16, 16), (50, 32, 18)]
    assert not r["reached"] and r["spp_done"] == 50 and len(r["history"]) == 4
    # a target met by the first batch; a first batch above max_spp
    ds = FakeScene(0.5)
    r = render.render_to_noise(ds, nx, ny, 256, 50, target=10.0, first_batch=4)
    assert ds.calls == [(256, 0, 4)] and r["reached"] and r["spp_done"] == 4
    ds = FakeScene(0.5)
    r = render.render_to_noise(ds, nx, ny, 5, 50, target=1e-6, first_batch=8)
    assert ds.calls == [(5, 0, 5)] and not r["reached"] and r["spp_done"] == 5
    for kw in ({"first_batch": 1}, {"max_spp": 1}, {"target": 0.0}, {"target": -1.0}, {"target": float("nan")}):
        args = {"max_spp": 64, "target": 0.1, "first_batch": 8, **kw}
        with pytest.raises(ValueError):
            render.render_to_noise(FakeScene(0.5), nx, ny, args.pop("max_spp"), 50, **args)


def declared_functions():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(rtw_[a-z_0-9]+)\s*\(", text)))


def test_header_and_abi_table(built, tmp_path):
    names = declared_functions()
    assert names == sorted(_abi.NOISE_SIGNATURES) and len(names) == 3
    assert not set(names) & set(_abi.SIGNATURES)
    lib = _abi.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_abi.LIB_PATH)], capture_output=True, text=True).stdout
    for n in names:
        assert hasattr(lib, n)
        assert re.search(rf"\bT {n}$", nm, re.M), f"{n} is not a defined text symbol"
    # the header is C11, and the struct's layout is the ctypes mirror's
    s = "rtw_noise_summary"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtw_noise.h"', "int main(void){",
             f'printf("{s} %zu\\n", sizeof({s}));']
    for f, _ in _abi.rtw_noise_summary._fields_:
        lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.split("\n") if l)
    assert int(out[s]) == C.sizeof(_abi.rtw_noise_summary) == 40
    for f, _ in _abi.rtw_noise_summary._fields_:
        assert int(out[f"{s}.{f}"]) == getattr(_abi.rtw_noise_summary, f).offset, f


def test_cli_refuses_bad_noise_options(built):
    """Decided from the arguments alone, before any device is touched."""
    cli = ROOT / "raytracingweekend_amd" / "rtw_render"
    for opts, word in ((["--noise", "--gpus", "2"], "one GPU"), (["--noise-target", "0.1", "--gpus", "2"], "one GPU"),
                       (["--noise-target", "0"], "--noise-target > 0"), (["--noise", "--spp", "1"], "--spp >= 2"),
                       (["--noise-target", "0.1", "--noise-batch", "1"], "--noise-batch >= 2"),
                       (["--noise", "--noise-floor", "0"], "--noise-floor > 0")):
        p = subprocess.run([str(cli), *opts], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and word in p.stderr, (opts, p.stdout, p.stderr)


def test_strict_build_exports_the_same_symbols(built):
    from raytracingweekend_amd import build
    if not build.STRICT_LIB.exists():
        pytest.fail(f"{build.STRICT_LIB} is missing: run `python -m raytracingweekend_amd.build` first")
    nm = subprocess.run(["nm", "-D", "--defined-only", str(build.STRICT_LIB)], capture_output=True, text=True).stdout
    for n in _abi.NOISE_SIGNATURES:
        assert re.search(rf"\bT {n}$", nm, re.M), f"{n} is not exported by the strict build"
