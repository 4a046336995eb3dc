"""Per-pixel noise estimate on the GPU (include/rtw_noise.h): the moments
render (k_reduce_moments) against its bit-exact definition over per-sample
renders, in every execution form, with rows / ranges / device buffers; the
device estimator against the host's; the render-to-target loop and the CLI.

"Per-sample renders" are render_accumulate(spp_begin=s, spp_count=1) into a
zero buffer: the existing path, which yields each sample's radiance exactly.
"""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle_lib import oracle_sums
from test_gpu_parity import TOL
from test_noise import FLOOR, moments_np, noise_np, same_bits

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "raytracingweekend_amd" / "rtw_render"


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


def per_sample(ds, nx, ny, spp, depth, seed, **kw):
    return [ds.render_accumulate(nx, ny, spp, depth, seed, spp_begin=s, spp_count=1, **kw)[0] for s in range(spp)]


@pytest.mark.parametrize("scene,bvh,nx,ny,spp,seed,precision", [
    ("cornell_box", False, 37, 23, 7, 3, "fp64"),   # 851 pixels: no multiple of 64; 7 = one batch of 4 + 3
    ("cornell_box", False, 37, 23, 7, 3, "fp32"),
    ("random_balls", True, 60, 40, 4, 7, "fp64"),
    ("random_balls", True, 60, 40, 4, 7, "fp32"),
    ("book2_final", False, 24, 24, 2, 7, "fp64"),
])
def test_moments_are_the_definition(gpu, scene, bvh, nx, ny, spp, seed, precision):
    ds = gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny, use_bvh=bvh))
    try:
        plain, st0 = ds.render_accumulate(nx, ny, spp, 50, seed, precision=precision)
        acc, sq, st = ds.render_moments(nx, ny, spp, 50, seed, precision=precision)
        xs = per_sample(ds, nx, ny, spp, 50, seed, precision=precision)
    finally:
        ds.close()
    s1, s2 = moments_np(xs)
    assert np.array_equal(acc, plain), "accum differs from rtw_render_accumulate's"
    assert np.array_equal(plain, s1)
    assert np.array_equal(sq, s2), f"max diff {np.abs(sq - s2).max()}"
    assert sq.any() and st["segments"] == st0["segments"] and st["samples"] == nx * ny * spp


def test_every_execution_form(gpu, monkeypatch):
    nx, ny, spp, depth, seed = 24, 24, 8, 50, 11
    ds = gpu.DeviceScene(gpu.SceneDesc("cornell_box", 1.0))
    try:
        a, q, _ = ds.render_moments(nx, ny, spp, depth, seed)
        monkeypatch.setenv("RTW_PASS_SAMPLES", str(nx * ny * 3))  # passes of 3 + 3 + 2 samples
        b, r, st = ds.render_moments(nx, ny, spp, depth, seed)
        assert st["launches_intersect"] == 3
        assert np.array_equal(a, b) and np.array_equal(q, r), "run2 must carry across passes"
        monkeypatch.delenv("RTW_PASS_SAMPLES")
        monkeypatch.setenv("RTW_MODE", "wavefront")
        b, r, _ = ds.render_moments(nx, ny, spp, depth, seed, wavefront_paths=1000)
        assert np.array_equal(a, b) and np.array_equal(q, r), "wavefront form"
        monkeypatch.setenv("RTW_SPLIT", "1")
        b, r, _ = ds.render_moments(nx, ny, spp, depth, seed, wavefront_paths=1000)
        assert np.array_equal(a, b) and np.array_equal(q, r), "split form"
    finally:
        ds.close()


def test_rows_ranges_and_add_semantics(gpu):
    nx, ny, spp, depth, seed = 32, 24, 6, 50, 3
    ds = gpu.DeviceScene(gpu.SceneDesc("cornell_box", nx / ny))
    try:
        sel = dict(row_begin=1, row_step=3, spp_begin=2, spp_count=3)
        z, zq, _ = ds.render_moments(nx, ny, spp, depth, seed, **sel)
        a, q = np.full(nx * ny * 3, 0.5), np.full(nx * ny * 3, 0.5)
        ds.render_moments(nx, ny, spp, depth, seed, accum=a, accum_sq=q, **sel)
        rows = np.zeros((ny, nx, 3), dtype=bool)
        rows[1::3] = True
        rows = rows.reshape(-1)
        assert (a[~rows] == 0.5).all() and (q[~rows] == 0.5).all()
        assert not z[~rows].any() and not zq[~rows].any() and zq[rows].any()
        assert np.array_equal(a[rows], 0.5 + z[rows]) and np.array_equal(q[rows], 0.5 + zq[rows])

        full, fullq, _ = ds.render_moments(nx, ny, spp, depth, seed)
        a, q = np.zeros_like(full), np.zeros_like(full)
        for r in range(3):
            ds.render_moments(nx, ny, spp, depth, seed, row_begin=r, row_step=3, accum=a, accum_sq=q)
        assert np.array_equal(a, full) and np.array_equal(q, fullq), "pixel sharding must be bit-exact"
        a, q = np.zeros_like(full), np.zeros_like(full)
        ds.render_moments(nx, ny, spp, depth, seed, spp_begin=0, spp_count=4, accum=a, accum_sq=q)
        ds.render_moments(nx, ny, spp, depth, seed, spp_begin=4, spp_count=2, accum=a, accum_sq=q)
        assert np.allclose(a, full, rtol=1e-12, atol=1e-12) and np.allclose(q, fullq, rtol=1e-12, atol=1e-12)
        # no samples / no depth: neither buffer is touched
        a, q = np.full(nx * ny * 3, 0.5), np.full(nx * ny * 3, 0.25)
        ds.render_moments(nx, ny, spp, 0, seed, accum=a, accum_sq=q)
        ds.render_moments(nx, ny, spp, depth, seed, spp_begin=spp, accum=a, accum_sq=q)
        assert (a == 0.5).all() and (q == 0.25).all()
    finally:
        ds.close()


def test_device_buffers(gpu):
    import torch
    from raytracingweekend_amd import _abi
    nx, ny, spp, depth, seed = 37, 23, 5, 50, 3
    n = nx * ny * 3
    sd = gpu.SceneDesc("cornell_box", nx / ny)
    ds = gpu.DeviceScene(sd)
    try:
        a, q, _ = ds.render_moments(nx, ny, spp, depth, seed)
        ta = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        tq = torch.zeros_like(ta)
        ds.render_moments(nx, ny, spp, depth, seed, accum=ta, accum_sq=tq)
        assert np.array_equal(ta.cpu().numpy(), a) and np.array_equal(tq.cpu().numpy(), q)
        # one buffer given: the partner is of its kind
        _, tq2, _ = ds.render_moments(nx, ny, spp, depth, seed, accum=torch.zeros_like(ta))
        assert tq2.is_cuda and np.array_equal(tq2.cpu().numpy(), q)
        with pytest.raises(ValueError, match="both"):
            ds.render_moments(nx, ny, spp, depth, seed, accum=ta, accum_sq=np.zeros(n))
        with pytest.raises(ValueError, match="both"):
            ds.noise_estimate(ta, np.zeros(n), nx, ny, spp)
        with pytest.raises(_abi.RtwError, match="overlap"):
            ds.render_moments(nx, ny, spp, depth, seed, accum=ta, accum_sq=ta)
        # through the C ABI: a device accum with a host accum_sq
        host = np.zeros(n)
        prm = _abi.rtw_render_params(nx=nx, ny=ny, spp=spp, max_depth=depth, seed=seed, row_step=1,
                                     accum_on_device=1)
        before = ta.clone()
        rc = _abi.lib().rtw_render_accumulate_moments(ds.handle, C.byref(sd.camera), C.byref(prm),
                                                      C.c_void_p(ta.data_ptr()), host.ctypes.data_as(C.c_void_p),
                                                      None)
        assert rc == -1 and b"not device" in _abi.lib().rtw_last_error()
        assert torch.equal(ta, before) and not host.any()
    finally:
        ds.close()


def test_grid_stride_path_of_the_reduction(gpu):
    """1200x900 pixels are more than reduce_grid's 4096 blocks of 256."""
    nx, ny, spp, depth, seed = 1200, 900, 2, 2, 1
    assert nx * ny > 4096 * 256
    ds = gpu.DeviceScene(gpu.SceneDesc("cornell_box", nx / ny))
    try:
        a, q, _ = ds.render_moments(nx, ny, spp, depth, seed)
        xs = per_sample(ds, nx, ny, spp, depth, seed)
    finally:
        ds.close()
    s1, s2 = moments_np(xs)
    assert np.array_equal(a, s1) and np.array_equal(q, s2) and q.any()


@pytest.mark.parametrize("scene,bvh,nx,ny,spp,depth", [("cornell_box", False, 40, 30, 4, 100),
                                                       ("random_balls", True, 60, 40, 4, 50),
                                                       ("book2_final", False, 24, 24, 2, 50)])
def test_stderr_matches_the_oracle(gpu, scene, bvh, nx, ny, spp, depth):
    """Cases of test_gpu_parity.CASES, seed 7: the standard-error map from the
    GPU's moments against the one from per-sample oracle renders, within the
    project's tolerance TOL = 1e-4 (measured on MI355X: see EXPERIMENTS.md)."""
    ds = gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny, use_bvh=bvh))
    try:
        a, q, st = ds.render_moments(nx, ny, spp, depth, seed=7)
    finally:
        ds.close()
    sd = gpu.SceneDesc(scene, nx / ny)
    outs = [oracle_sums(sd, nx, ny, spp, depth, seed=7, spp_begin=s, spp_count=1) for s in range(spp)]
    s1, s2 = moments_np([o[0] for o in outs])
    assert st["segments"] == sum(o[1] for o in outs), "device-counted traversals differ from the oracle's"
    se_gpu, _ = gpu.noise_estimate(a, q, nx, ny, spp, FLOOR)
    se_ref, _ = gpu.noise_estimate(s1, s2, nx, ny, spp, FLOOR)
    assert np.isfinite(se_gpu).all() and se_ref.any()
    d = np.abs(se_gpu - se_ref)
    print(f"{scene} {nx}x{ny}x{spp}: max |stderr diff| vs oracle = {d.max():.3e}, max stderr {se_ref.max():.3e}")
    assert d.max() <= TOL


def check_device_estimator(ds, s1, s2, nx, ny, n):
    import torch
    t1 = torch.from_numpy(s1).to("cuda:0")
    t2 = torch.from_numpy(s2).to("cuda:0")
    se_h, sum_h = ds.noise_estimate(s1, s2, nx, ny, n, FLOOR)  # numpy: the host function
    se_d, sum_d = ds.noise_estimate(t1, t2, nx, ny, n, FLOOR)
    assert se_d.is_cuda
    assert same_bits(se_d.cpu().numpy(), se_h), "device stderr map differs from the host's"
    assert sum_d["pixels"] == sum_h["pixels"] and sum_d["nonfinite"] == sum_h["nonfinite"]
    assert sum_d["pixels"] + sum_d["nonfinite"] == nx * ny
    for k in ("mean_rel", "max_rel", "rms_stderr"):
        assert sum_d[k] == pytest.approx(sum_h[k], rel=1e-9), k
    assert sum_d["max_rel"] == sum_h["max_rel"]
    se_d2, sum_d2 = ds.noise_estimate(t1, t2, nx, ny, n, FLOOR)
    assert sum_d2 == sum_d and torch.equal(se_d2.view(torch.int64), se_d.view(torch.int64)), "not deterministic"
    none, sum_d3 = ds.noise_estimate(t1, t2, nx, ny, n, FLOOR, want_stderr=False)
    assert none is None and sum_d3 == sum_d
    want_se, want = noise_np(s1, s2, n)
    assert same_bits(se_h, want_se) and sum_h["pixels"] == want["pixels"]
    return sum_d


def test_device_estimator(gpu):
    import torch
    from raytracingweekend_amd import _abi
    nx, ny, spp = 37, 23, 7
    ds = gpu.DeviceScene(gpu.SceneDesc("cornell_box", nx / ny))
    try:
        a, q, _ = ds.render_moments(nx, ny, spp, 50, seed=3)
        s = check_device_estimator(ds, a, q, nx, ny, spp)
        assert s["nonfinite"] == 0 and s["mean_rel"] > 0
        a2, q2 = a.copy(), q.copy()
        a2[3 * 100 + 1] = np.nan
        a2[3 * 500] = q2[3 * 500] = np.inf
        s = check_device_estimator(ds, a2, q2, nx, ny, spp)
        assert s["nonfinite"] == 2
        s = check_device_estimator(ds, np.full(3, np.nan), np.ones(3), 1, 1, 4)
        assert s == {"pixels": 0, "nonfinite": 1, "mean_rel": 0.0, "max_rel": 0.0, "rms_stderr": 0.0}
        # 1 pixel; 2100 pixels (9 blocks, the last one partly filled); 300 000
        # pixels (more than the 1024 blocks of 256 the grid is capped at)
        for w, h, n in ((1, 1, 5), (300, 7, 7), (600, 500, 3)):
            rng = np.random.default_rng([w, h])
            xs = list(rng.random((n, w * h * 3)) * rng.random(w * h * 3) * 3.0)
            s1, s2 = moments_np(xs)
            s = check_device_estimator(ds, s1, s2, w, h, n)
            assert s["pixels"] == w * h
        # argument errors of the device entry point
        t = torch.zeros(nx * ny * 3, dtype=torch.float64, device="cuda:0")
        with pytest.raises(_abi.RtwError, match="overlap"):
            ds.noise_estimate(t, t, nx, ny, spp)
        with pytest.raises(_abi.RtwError, match="n >= 2"):
            ds.noise_estimate(t, torch.zeros_like(t), nx, ny, 1)
    finally:
        ds.close()


@pytest.fixture(scope="module")
def balls(gpu):
    """random_balls 60x40, depth 50, seed 7: mean_rel after samples [0,8) and
    [0,64), and a target between them."""
    nx, ny, depth, seed = 60, 40, 50, 7
    ds = gpu.DeviceScene(gpu.SceneDesc("random_balls", nx / ny))
    try:
        r = {}
        for n in (8, 64):
            a, q, _ = ds.render_moments(nx, ny, 256, depth, seed, spp_begin=0, spp_count=n)
            r[n] = ds.noise_estimate(a, q, nx, ny, n, FLOOR, want_stderr=False)[1]["mean_rel"]
    finally:
        ds.close()
    print(f"random_balls 60x40: mean_rel {r[8]:.4f} at 8 spp, {r[64]:.4f} at 64 spp")
    assert r[64] < r[8]
    return dict(nx=nx, ny=ny, depth=depth, seed=seed, target=float(np.sqrt(r[8] * r[64])))


@pytest.mark.parametrize("device_buffers", [False, True])
def test_render_to_target(gpu, balls, device_buffers):
    nx, ny, depth, seed, target = (balls[k] for k in ("nx", "ny", "depth", "seed", "target"))
    ds = gpu.DeviceScene(gpu.SceneDesc("random_balls", nx / ny))
    try:
        r = gpu.render_to_noise(ds, nx, ny, 256, depth, seed, target=target, first_batch=8,
                                device_buffers=device_buffers)
        n = r["spp_done"]
        a, q, _ = ds.render_moments(nx, ny, 256, depth, seed, spp_begin=0, spp_count=n)
    finally:
        ds.close()
    assert r["reached"] and 8 < n <= 64
    assert [h[0] for h in r["history"]] == [8, 16, 32, 64][:len(r["history"])] and r["history"][-1][0] == n
    assert r["history"][-1][1] <= target and all(h[1] > target for h in r["history"][:-1])
    assert r["stats"]["samples"] == nx * ny * n
    got_a, got_q = r["accum"], r["accum_sq"]
    if device_buffers:
        assert got_a.is_cuda and got_q.is_cuda
        got_a, got_q = got_a.cpu().numpy(), got_q.cpu().numpy()
    assert np.allclose(got_a, a, rtol=1e-12, atol=1e-12) and np.allclose(got_q, q, rtol=1e-12, atol=1e-12)


def test_cli(gpu, balls, tmp_path):
    nx, ny, depth, seed, target = (balls[k] for k in ("nx", "ny", "depth", "seed", "target"))
    ds = gpu.DeviceScene(gpu.SceneDesc("random_balls", nx / ny))
    try:
        r = gpu.render_to_noise(ds, nx, ny, 64, depth, seed, target=target, first_batch=8)
    finally:
        ds.close()
    out = tmp_path / "n.ppm"
    base = [str(CLI), "--scene", "random_balls", "--nx", str(nx), "--ny", str(ny), "--spp", "64", "--depth",
            str(depth), "--seed", str(seed)]
    p = subprocess.run(base + ["--noise-target", repr(target), "--out", str(out)], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"^Noise: spp (\d+) of 64  mean_rel (\S+)  max_rel (\S+)  rms_stderr (\S+)$", p.stdout, re.M)
    assert m, p.stdout
    assert int(m.group(1)) == r["spp_done"]
    assert float(m.group(2)) == pytest.approx(r["history"][-1][1], rel=1e-5)
    canvas = gpu.finalize(r["accum"], nx, ny, r["spp_done"])
    want = (np.float64(np.float32(255.99)) * canvas).astype(np.int64).reshape(ny, nx, 3)[::-1].reshape(-1)
    tok = out.read_text().split()
    assert tok[:4] == ["P3", str(nx), str(ny), "255"]
    got = np.array(tok[4:], dtype=np.int64)
    assert got.size == want.size and (got != want).sum() <= max(1, want.size // 10000)
    # --noise alone: all the samples, one line
    p = subprocess.run(base[:-6] + ["--spp", "4", "--depth", "10", "--noise", "--out", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and re.search(r"^Noise: spp 4 of 4  mean_rel ", p.stdout, re.M), p.stdout + p.stderr
    # one GPU only
    for opt in (["--noise"], ["--noise-target", "0.1"]):
        p = subprocess.run(base + opt + ["--gpus", "2", "--out", str(out)], capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 2 and "one GPU" in p.stderr, p.stdout + p.stderr
