"""The denoiser (include/rtw_denoise.h), CPU side: the header and ABI table,
the host filter against a second statement of it in numpy written from the
header's text, its exact edges, pass-through pixels and constant images, that
noise actually falls, and the host code under AddressSanitizer / UBSan
(tests/cpp/denoise_check.cpp, a program of its own: nothing is preloaded).
No GPU compute here."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from raytracingweekend_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "raytracingweekend_amd" / "csrc"
HOST = CSRC / "host"
HEADER = ROOT / "include" / "rtw_denoise.h"
DEFAULTS = dict(iterations=5, sigma_l=4.0, sigma_z=0.1, eps_a=1e-2, normal_power_log2=7)


@pytest.fixture(scope="module")
def render(built):
    from raytracingweekend_amd import render
    return render


# ---- the filter a second time, from the header's text ---------------------------
def _shift(a, dy, dx):
    """a[j + dy, i + dx] for every (j, i), and the mask of taps inside the image."""
    ny, nx = a.shape[:2]
    jj = np.arange(ny)[:, None] + dy
    ii = np.arange(nx)[None, :] + dx
    inside = (jj >= 0) & (jj < ny) & (ii >= 0) & (ii < nx)
    return a[np.clip(jj, 0, ny - 1), np.clip(ii, 0, nx - 1)], inside


def denoise_np(s1, s2, counts, f, fs, nx, ny, iterations, sigma_l, sigma_z, eps_a, normal_power_log2):
    """rtw_denoise.h's PREPARE / ITERATE / FINISH, vectorised per tap.  Returns
    (out, out_var), each (ny, nx, 3)."""
    s1 = np.asarray(s1, dtype=np.float64).reshape(ny, nx, 3)
    s2 = np.asarray(s2, dtype=np.float64).reshape(ny, nx, 3)
    f = np.asarray(f, dtype=np.float64).reshape(ny, nx, 8)
    n = np.asarray(counts).reshape(ny, nx, 1).astype(np.float64)
    with np.errstate(all="ignore"):
        m = s1 / n
        v = (s2 - s1 * m) / (n - 1.0)
        v = np.where(v < 0, 0.0, v) / n
        valid = (n[..., 0] >= 2) & np.isfinite(s1).all(-1) & np.isfinite(s2).all(-1)
        if iterations == 0:
            return m, np.where(valid[..., None], v, np.nan)
        a = f[..., 0:3] / fs + eps_a
        N = f[..., 3:6] / fs
        d = f[..., 6] / fs
        cov = f[..., 7] / fs
        ln = np.sqrt((N ** 2).sum(-1))
        N = np.where(ln[..., None] > 0, N / np.where(ln > 0, ln, 1.0)[..., None], N)
        valid = valid & np.isfinite(f).all(-1) & (a > 0).all(-1)
        c = np.where(valid[..., None], m / a, m)
        v = v / (a * a)
        has_n = (N != 0).any(-1)
        h = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])

        def wn_of(dy, dx):
            Nq, _ = _shift(N, dy, dx)
            hq, _ = _shift(has_n, dy, dx)
            dot = np.maximum((N * Nq).sum(-1), 0.0) ** (2 ** normal_power_log2)
            return np.where(has_n & hq, dot, np.where(has_n | hq, 0.0, 1.0))

        for k in range(iterations):
            step = 2 ** k
            l, lv = c.sum(-1) / 3.0, v.sum(-1) / 9.0
            gs, gw = np.zeros((ny, nx)), np.zeros((ny, nx))
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    lvq, inside = _shift(lv, dy, dx)
                    vq, _ = _shift(valid, dy, dx)
                    cq, _ = _shift(cov, dy, dx)
                    on = inside & vq & (np.abs(cov - cq) <= 0.5) & (wn_of(dy, dx) > 0)
                    wg = (2 - abs(dy)) * (2 - abs(dx))
                    gs += np.where(on, wg * lvq, 0.0)
                    gw += np.where(on, wg, 0.0)
            den = sigma_l * np.sqrt(gs / gw) + 1e-12
            sw, sc, sv = np.zeros((ny, nx)), np.zeros((ny, nx, 3)), np.zeros((ny, nx, 3))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * step, dx * step
                    lq, inside = _shift(l, oy, ox)
                    vq, _ = _shift(valid, oy, ox)
                    covq, _ = _shift(cov, oy, ox)
                    dq, _ = _shift(d, oy, ox)
                    ccq, _ = _shift(c, oy, ox)
                    vvq, _ = _shift(v, oy, ox)
                    xl = np.abs(l - lq) / den
                    xz = np.abs(d - dq) / (sigma_z * (d + dq) + 1e-12)
                    x = xl + xz  # exp_neg: exp(-x) for x <= 64, 0 above
                    w = h[dy + 2] * h[dx + 2] * np.where(x <= 64.0, np.exp(-x), 0.0) * wn_of(oy, ox)
                    on = inside & vq & (np.abs(cov - covq) <= 0.5) & (w > 0)
                    w = np.where(on, w, 0.0)
                    sw += w
                    sc += np.where(on[..., None], w[..., None] * ccq, 0.0)
                    sv += np.where(on[..., None], (w * w)[..., None] * vvq, 0.0)
            c = np.where(valid[..., None], sc / sw[..., None], c)
            v = np.where(valid[..., None], sv / (sw * sw)[..., None], v)
        out = np.where(valid[..., None], c * a, m)
        var = np.where(valid[..., None], v * (a * a), np.nan)
    return out, var


def random_image(nx, ny, seed, n=8, fs=4):
    """Random moments of n samples and plausible features: two normals, a sky
    region, varying depth and albedo."""
    rng = np.random.default_rng([seed, nx, ny])
    npix = nx * ny
    mean = 0.2 + rng.random((npix, 3))
    sd = 0.4 * rng.random((npix, 3))
    s1 = mean * n
    s2 = (mean ** 2 + sd ** 2) * n
    f = np.zeros((npix, 8))
    i = np.arange(npix) % nx
    j = np.arange(npix) // nx
    sky = (j < ny // 4) & (i > nx // 2)
    tilt = np.where(i < nx // 3, 0.0, 0.3)[:, None] * rng.random((npix, 1))
    normal = np.stack([tilt[:, 0], np.zeros(npix), np.sqrt(1 - tilt[:, 0] ** 2)], axis=1)
    cov = np.where(sky, 0.0, 1.0)
    f[:, 0:3] = (0.1 + 0.8 * rng.random((npix, 3))) * fs
    f[:, 3:6] = normal * cov[:, None] * fs
    f[:, 6] = (0.2 + 0.02 * rng.random(npix)) * cov * fs
    f[:, 7] = cov * fs
    return s1.reshape(-1), s2.reshape(-1), f.reshape(-1), n, fs


def rel_err(got, want):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    ok = np.isfinite(want)
    assert np.array_equal(got[~ok], want[~ok], equal_nan=True), "NaN / Inf in different places"
    return float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)))


# ---- tests ------------------------------------------------------------------------
def test_header_adds_symbols_only_and_the_abi_table_has_them(built):
    text = HEADER.read_text()
    import re
    names = set(re.findall(r"\b(rtw_[a-z_]+)\s*\(", text.split("#ifndef RTW_DENOISE_H")[1]))
    assert names == set(_abi.DENOISE_SIGNATURES), names ^ set(_abi.DENOISE_SIGNATURES)
    assert _abi.RTW_ABI_VERSION == 4 and _abi.lib().rtw_abi_version() == 4
    import ctypes as C
    assert C.sizeof(_abi.rtw_denoise_params) == 32
    nm = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "raytracingweekend_amd" / "librtw.so")],
                        capture_output=True, text=True).stdout
    for name in _abi.DENOISE_SIGNATURES:
        assert f" T {name}\n" in nm, name


def test_defaults(render):
    prm = render.denoise_params()
    assert {k: getattr(prm, k) for k in DEFAULTS} == DEFAULTS
    with pytest.raises(ValueError):
        render.denoise_params(sigma=1.0)


@pytest.mark.parametrize("with_counts", [False, True])
def test_zero_iterations_is_the_mean(render, with_counts):
    """iterations = 0 returns S1 / n bit for bit (S1 / counts[p] with counts)."""
    nx, ny = 13, 7
    s1, s2, f, n, fs = random_image(nx, ny, 1)
    counts = (2 + np.arange(nx * ny) % 7).astype(np.uint32) if with_counts else None
    out, var = render.denoise(s1, s2, f, nx, ny, n=n, counts=counts, feature_spp=fs, want_variance=True, iterations=0)
    den = np.repeat(counts, 3).astype(np.float64) if with_counts else float(n)
    assert np.array_equal(out, s1 / den)
    want_var = denoise_np(s1, s2, counts if with_counts else np.full(nx * ny, n), f, fs, nx, ny, 0, 4, .1, .01, 7)[1]
    assert np.array_equal(var, want_var.reshape(-1))


def test_constant_image_stays_constant(render):
    """A constant colour with any variance and flat features comes back as the
    constant within 25 * 8 * 2^-53 relative."""
    nx, ny, n, fs = 37, 23, 8, 4
    rng = np.random.default_rng(4)
    npix = nx * ny
    s1 = np.full(npix * 3, 0.625 * n)
    s2 = s1 * 0.625 + n * rng.random(npix * 3) ** 2 * 3.0
    f = np.tile(np.array([0.5, 0.5, 0.5, 0, 0, 1, 0.25, 1]) * fs, npix)
    out = render.denoise(s1, s2, f, nx, ny, n=n, feature_spp=fs)
    assert np.max(np.abs(out - 0.625) / 0.625) <= 25 * 8 * 2.0 ** -53


def test_pass_through_pixels_are_outside_the_image(render):
    """A NaN pixel and a count-1 pixel come out as m and are no tap: with the
    last column made of them, every other pixel's output is bit for bit that of
    the image without that column."""
    nx, ny = 20, 9
    s1, s2, f, n, fs = random_image(nx, ny, 2)
    counts = np.full(nx * ny, n, dtype=np.uint32)
    s1 = s1.copy()
    last = np.arange(ny) * nx + nx - 1
    counts[last[0::2]] = 1
    s1[3 * last[1::2] + 1] = np.nan
    out, var = render.denoise(s1, s2, f, nx, ny, counts=counts, feature_spp=fs, want_variance=True)
    keep = np.ones(nx * ny, dtype=bool)
    keep[last] = False
    crop = lambda a, k: a.reshape(ny, nx, k)[:, :nx - 1].reshape(-1).copy()
    out_c, var_c = render.denoise(crop(s1, 3), crop(s2, 3), crop(f, 8), nx - 1, ny, counts=counts[keep].copy(),
                                  feature_spp=fs, want_variance=True)
    assert np.array_equal(crop(out, 3), out_c) and np.array_equal(crop(var, 3), var_c)
    o = out.reshape(-1, 3)
    m = s1.reshape(-1, 3) / counts[:, None]
    assert np.array_equal(o[last], m[last], equal_nan=True) and np.isnan(var.reshape(-1, 3)[last]).all()
    assert np.isnan(o[last[1::2], 1]).all() and np.isfinite(o[last[0::2]]).all()
    # ... and a pixel without samples is NaN
    counts[5] = 0
    out0 = render.denoise(s1, s2, f, nx, ny, counts=counts, feature_spp=fs)
    assert np.isnan(out0.reshape(-1, 3)[5]).all()


@pytest.mark.parametrize("iterations", [1, 5])
def test_against_the_numpy_restatement(render, iterations):
    """37x23, 5 iterations: the last step, 16, exceeds half the height, so taps
    fall off both edges; a NaN pixel, a count-1 pixel and a sky region inside.
    Agreement within 1e-12 relative, means and variances."""
    nx, ny = 37, 23
    s1, s2, f, n, fs = random_image(nx, ny, 3)
    counts = (2 + np.arange(nx * ny) % 9).astype(np.uint32)
    counts[100] = 1
    s1 = s1.copy()
    s1[3 * 333] = np.inf
    for cn in (counts, None):
        prm = dict(DEFAULTS, iterations=iterations)
        out, var = render.denoise(s1, s2, f, nx, ny, n=n, counts=cn, feature_spp=fs, want_variance=True, **prm)
        want, want_var = denoise_np(s1, s2, cn if cn is not None else np.full(nx * ny, n), f, fs, nx, ny, **prm)
        e, ev = rel_err(out, want), rel_err(var, want_var)
        print(f"iterations {iterations} counts {cn is not None}: mean {e:.3e} variance {ev:.3e}")
        assert e <= 1e-12 and ev <= 1e-12


def synthetic_noise(nx, ny, n, sigma, seed):
    rng = np.random.default_rng(seed)
    x = 1.0 + sigma * rng.standard_normal((n, nx * ny * 3))
    f = np.tile(np.array([0.5, 0.5, 0.5, 0, 0, 1, 0.25, 1]) * n, nx * ny)
    return x.sum(0), (x * x).sum(0), f


def test_noise_falls_and_the_variance_map_follows(render):
    """Flat features, colour 1 + iid noise of variance sigma^2 per sample: the
    output's sample variance is below the input's (sigma^2 / n) after the
    default 5 passes, and after one pass -- where the taps are independent, as
    the propagation v' = sum w^2 v / (sum w)^2 assumes -- the returned variance
    map is within a factor 2 of the output's sample variance.  (Later passes
    read neighbours that share inputs: the map then underestimates, as the
    header says; the ratio is printed.)"""
    nx, ny, n, sigma = 64, 48, 16, 0.5
    s1, s2, f = synthetic_noise(nx, ny, n, sigma, 7)
    var_in = float(np.var(s1 / n))
    ratios = {}
    for it in (1, 5):
        out, var = render.denoise(s1, s2, f, nx, ny, n=n, feature_spp=n, want_variance=True, iterations=it)
        var_out = float(np.mean((out - 1.0) ** 2))
        ratios[it] = (var_out / var_in, float(var.mean()) / var_out)
        print(f"iterations {it}: output variance / input variance {ratios[it][0]:.4f}, "
              f"variance map / output variance {ratios[it][1]:.4f}")
        assert var_out < var_in
    assert 0.5 <= ratios[1][1] <= 2.0
    assert ratios[5][0] < ratios[1][0]


def test_python_argument_errors(render):
    nx, ny = 6, 5
    s1, s2, f, n, fs = random_image(nx, ny, 5)
    for bad in (dict(iterations=9), dict(iterations=-1), dict(sigma_l=0.0), dict(sigma_z=float("nan")), dict(eps_a=0.0)):
        with pytest.raises(_abi.RtwError):
            render.denoise(s1, s2, f, nx, ny, n=n, feature_spp=fs, **bad)
    with pytest.raises(_abi.RtwError):
        render.denoise(s1, s2, f, nx, ny, n=1, feature_spp=fs)
    with pytest.raises(_abi.RtwError):
        render.denoise(s1, s2, f, nx, ny, n=n, feature_spp=0)
    with pytest.raises(ValueError):
        render.denoise(s1, s2, f[:-8], nx, ny, n=n, feature_spp=fs)
    assert np.array_equal(render.finalize_mean(np.array([0.25, 4.0, 0.0]), 1, 1), [0.5, 1.0, 0.0])


FLAVOURS = {"plain": ["-O1"],
            "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                          "-O1"]}


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_denoise_host_code(tmp_path, flavour):
    """tests/cpp/denoise_check.cpp over denoise.cpp: exp_neg and pow2k, the
    exact normal and coverage edges, every argument error, iterations 0 and
    the shapes whose taps fall off the image; built plainly and with
    -fsanitize=address,undefined and run directly."""
    inc = [f"-I{ROOT / 'include'}", f"-I{CSRC}", f"-I{HOST}"]
    exe = tmp_path / "denoise_check"
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", *FLAVOURS[flavour], *inc,
           str(ROOT / "tests" / "cpp" / "denoise_check.cpp"), *[str(HOST / s) for s in ("denoise.cpp", "output.cpp")],
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "OK (denoise_check)", (r.stdout + r.stderr)[-4000:]


def test_cli_refuses_bad_denoise_options(built):
    """Decided from the arguments alone, before any device is touched."""
    cli = ROOT / "raytracingweekend_amd" / "rtw_render"
    for opts in (["--denoise", "--gpus", "2"], ["--denoise", "--spp", "1"], ["--denoise-iterations", "9"]):
        p = subprocess.run([str(cli), *opts], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "--denoise" in p.stderr, (opts, p.stdout, p.stderr)
