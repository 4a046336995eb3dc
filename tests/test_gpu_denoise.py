"""The denoiser on the GPU (include/rtw_denoise.h): the device filter against
the host function bit for bit, the first-hit feature sums against the host
classes (tests/cpp/host_features.cpp) and against the reference-derived
Normal-mode goldens, their additivity, the end-to-end gain over the raw render,
the adaptive pairing and rtw_render --denoise.  All renders use depth 50."""
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_denoise import DEFAULTS, random_image

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "raytracingweekend_amd"
GOLD = ROOT / "tests" / "golden"
CLI = PKG / "rtw_render"
CASES = {c["case"]: c for c in json.loads((GOLD / "renders.json").read_text())}
DEPTH = 50
F_MEDIA, F_WBVH, F_GBVH = 1, 2, 4


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


@pytest.fixture(scope="module")
def ds_any(gpu):
    """A handle for the calls that read no scene (the filter's scratch)."""
    ds = gpu.DeviceScene(gpu.SceneDesc("cornell_box", 1.0))
    yield ds
    ds.close()


def to_dev(a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).cuda()


# ---- 9. the device filter is the host filter, bit for bit ---------------------------
@pytest.mark.parametrize("size", [(1, 1), (1, 70), (37, 23), (65, 17), (130, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("iterations", [1, 3, 5])
def test_device_filter_is_the_host_filter(gpu, ds_any, size, iterations):
    """1x1, 1x70, 37x23, 65x17, 130x5: the smallest shapes that cross a tile
    edge (32x8) in x, in y, in both, and that are thinner than a halo; uniform
    n and counts; a NaN pixel and a count-1 pixel inside.  Steps 1 and 2 run
    the LDS-tile kernel and the later ones the global kernel, so 3 iterations
    cover the switch."""
    import torch
    nx, ny = size
    s1, s2, f, n, fs = random_image(nx, ny, 9)
    counts = (2 + np.arange(nx * ny) % 9).astype(np.uint32)
    s1 = s1.copy()
    if nx * ny > 3:
        counts[(nx * ny) // 3] = 1
        s1[3 * ((nx * ny) // 2) + 2] = np.nan
    prm = dict(DEFAULTS, iterations=iterations)
    d1, d2, df = to_dev(s1), to_dev(s2), to_dev(f)
    for cn in (None, counts):
        want, want_var = gpu.denoise(s1, s2, f, nx, ny, n=n, counts=cn, feature_spp=fs, want_variance=True, **prm)
        dc = to_dev(cn.astype(np.int32)) if cn is not None else None
        out, var = ds_any.denoise(d1, d2, df, nx, ny, n=n, counts=dc, feature_spp=fs, want_variance=True, **prm)
        torch.cuda.synchronize()
        what = f"{nx}x{ny} iterations {iterations} counts {cn is not None}"
        assert np.array_equal(out.cpu().numpy(), want, equal_nan=True), what
        assert np.array_equal(var.cpu().numpy(), want_var, equal_nan=True), what
    # ... and iterations 0, and the canvas step
    out0 = ds_any.denoise(d1, d2, df, nx, ny, n=n, feature_spp=fs, iterations=0)
    assert np.array_equal(out0.cpu().numpy(), s1 / n, equal_nan=True)
    pos = torch.abs(out0)
    assert np.array_equal(ds_any.finalize_mean(pos, nx, ny).cpu().numpy(), gpu.finalize_mean(pos.cpu().numpy(), nx, ny),
                          equal_nan=True)


def test_device_filter_refuses_what_the_host_refuses(gpu, ds_any):
    from raytracingweekend_amd._abi import RtwError
    nx, ny = 6, 5
    s1, s2, f, n, fs = random_image(nx, ny, 5)
    d1, d2, df = to_dev(s1), to_dev(s2), to_dev(f)
    for bad in (dict(iterations=9), dict(sigma_l=0.0), dict(sigma_z=float("nan")), dict(eps_a=-1.0)):
        with pytest.raises(RtwError):
            ds_any.denoise(d1, d2, df, nx, ny, n=n, feature_spp=fs, **bad)
    with pytest.raises(RtwError):
        ds_any.denoise(d1, d2, df, nx, ny, n=1, feature_spp=fs)


# ---- 10. features against the host classes -----------------------------------------------
def _compile(src, exe):
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", f"-I{ROOT / 'include'}",
           f"-I{PKG / 'csrc' / 'host'}", f"-I{PKG / 'csrc' / 'host' / 'rtw'}", str(ROOT / "tests" / "cpp" / src),
           f"-L{PKG}", "-lrtw", f"-Wl,-rpath,{PKG}", "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def host_features(built, tmp_path_factory):
    exe = _compile("host_features.cpp", tmp_path_factory.mktemp("host_features") / "host_features")
    cache = {}

    def run(scene, nx, ny, spp, seed):
        """(feature sums nx*ny*8, textured-hit counts nx*ny) of the host classes, once per case."""
        key = (scene, nx, ny, spp, seed)
        if key not in cache:
            out = exe.parent / ("_".join(map(str, key)) + ".bin")
            r = subprocess.run([str(exe), scene, str(nx), str(ny), str(spp), str(seed), str(out)], capture_output=True,
                               text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            raw = np.fromfile(out, dtype=np.float64)
            f, t = raw[:nx * ny * 8].copy(), raw[nx * ny * 8:].copy()
            f.setflags(write=False), t.setflags(write=False)
            cache[key] = (f, t)
        return cache[key]
    return run


FEATURE_CASES = [("cornell_box", False, 32, 32, 4, 0), ("random_balls", False, 32, 24, 4, 0),
                 ("random_balls", True, 32, 24, 4, F_WBVH), ("book2_final", False, 16, 16, 2, F_MEDIA),
                 ("book2_final", True, 16, 16, 2, F_MEDIA | F_GBVH), ("textured", False, 24, 16, 4, 0),
                 ("textured", True, 24, 16, 4, F_WBVH), ("nested", False, 24, 24, 4, F_MEDIA),
                 ("grouped", True, 32, 24, 2, F_GBVH),
                 ("grouped_world", True, 32, 24, 2, F_WBVH | F_GBVH)]


@pytest.mark.parametrize("scene,bvh,nx,ny,spp,form", FEATURE_CASES,
                         ids=[f"{c[0]}-{'bvh' if c[1] else 'flat'}" for c in FEATURE_CASES])
def test_features_match_the_host_classes(gpu, host_features, scene, bvh, nx, ny, spp, form):
    """The eight sums of every pixel against tests/cpp/host_features.cpp (the
    same streams, hittable::hit of the host classes): coverage exact, albedo,
    normals and inverse depth within 1e-13 (the project's canvas parity
    figure), relative to 1 or the value.  The cases reach all six traversal
    forms of k_features: 0, media, world BVH, group BVH, media + group BVH,
    world + group BVH."""
    seed = 7
    ref, _ = host_features(scene, nx, ny, spp, seed)
    ds = gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny, use_bvh=bvh))
    try:
        got, st = ds.render_features(nx, ny, spp, seed)
        name = ds.query_features()
        info = ds.query()
    finally:
        ds.close()
    print(f"{scene} {'bvh' if bvh else 'flat'}: {name}  (render: {info['kernel']})")
    assert name == f"k_features<{form}>", name
    assert st["samples"] == nx * ny * spp and st["segments"] == st["samples"]
    g, r = got.reshape(-1, 8), ref.reshape(-1, 8)
    assert np.array_equal(g[:, 7], r[:, 7]), "coverage"
    err = np.abs(g[:, :7] - r[:, :7]) / np.maximum(np.abs(r[:, :7]), 1.0)
    print(f"  max error: albedo {err[:, :3].max():.3e} normal {err[:, 3:6].max():.3e} 1/t {err[:, 6].max():.3e}")
    assert err.max() <= 1e-13


def test_features_do_not_read_depth_precision_or_render_type(gpu):
    """max_depth and precision are not read: the C entry point with depth 0 and
    fp32 gives the bits of the Python wrapper's call."""
    import ctypes as C
    from raytracingweekend_amd import _abi
    nx, ny, spp, seed = 24, 16, 3, 5
    ds = gpu.DeviceScene(gpu.SceneDesc("random_balls", nx / ny))
    try:
        want, _ = ds.render_features(nx, ny, spp, seed)
        got = np.zeros_like(want)
        prm = _abi.rtw_render_params(nx=nx, ny=ny, spp=spp, max_depth=0, seed=seed, row_step=1,
                                     precision=_abi.PRECISIONS["fp32"])
        cam = ds.scene.camera
        _abi.check(_abi.lib().rtw_render_features(ds.handle, C.byref(cam), C.byref(prm), got.ctypes.data_as(C.c_void_p),
                                                  None), "rtw_render_features")
    finally:
        ds.close()
    assert np.array_equal(got, want)


# ---- 11. features against the reference-derived goldens -----------------------------------
@pytest.mark.parametrize("case", ["cornell_normal_32x32x4", "book2_final_normal_16x16x2", "nested_normal_24x24x4",
                                  "random_balls_normal_48x32x4"])
def test_normals_match_the_reference_goldens(gpu, case):
    """The Normal-mode goldens hold, per pixel, the sum over its samples of
    0.5 (normal + 1) of a hit and the background's colour of a miss, made by
    the reference's own classes: 0.5 (normal sum + coverage) equals them within
    1e-13 where no sample missed -- every pixel of a black-background scene's
    golden whose misses add 0, and the pixels with coverage == spp of a
    gradient-background one, which are at least a quarter of the image."""
    c = CASES[case]
    nx, ny, spp = c["nx"], c["ny"], c["spp"]
    gold = np.load(GOLD / f"render_{case}.npy").reshape(-1, 3)
    sd = gpu.SceneDesc(c["scene"], nx / ny)
    ds = gpu.DeviceScene(sd)
    try:
        f, _ = ds.render_features(nx, ny, spp, c["seed"])
        black = sd.desc.background != 1  # RTW_BG_GRADIENT
    finally:
        ds.close()
    f = f.reshape(-1, 8)
    full = f[:, 7] == spp
    use = np.ones(nx * ny, dtype=bool) if black else full
    print(f"{case}: background {'black' if black else 'gradient'}, fully covered {full.mean():.3f} of the image")
    assert use.mean() >= 0.25
    got = 0.5 * (f[:, 3:6] + f[:, 7:8])
    assert np.max(np.abs(got[use] - gold[use])) <= 1e-13


# ---- 12. additivity ----------------------------------------------------------------------
@pytest.mark.parametrize("scene,bvh", [("cornell_box", False), ("random_balls", True)])
def test_feature_sums_add_up_bit_for_bit(gpu, scene, bvh):
    """Samples [0, 2) and [2, 4) into one buffer are samples [0, 4); three row
    shards are the whole image; host buffers and device tensors alike."""
    import torch
    nx, ny, spp, seed = 33, 21, 4, 11
    ds = gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny, use_bvh=bvh))
    try:
        whole, _ = ds.render_features(nx, ny, spp, seed)
        parts = np.zeros_like(whole)
        ds.render_features(nx, ny, spp, seed, spp_begin=0, spp_count=2, features=parts)
        ds.render_features(nx, ny, spp, seed, spp_begin=2, spp_count=2, features=parts)
        rows = np.zeros_like(whole)
        for k in range(3):
            ds.render_features(nx, ny, spp, seed, row_begin=k, row_step=3, features=rows)
        dev = torch.zeros(nx * ny * 8, dtype=torch.float64, device="cuda")
        ds.render_features(nx, ny, spp, seed, spp_count=1, features=dev)
        ds.render_features(nx, ny, spp, seed, spp_begin=1, features=dev)
        torch.cuda.synchronize()
    finally:
        ds.close()
    assert whole.any()
    assert np.array_equal(parts, whole) and np.array_equal(rows, whole) and np.array_equal(dev.cpu().numpy(), whole)


# ---- 13. end to end --------------------------------------------------------------------------
def rmse(a, b, mask=None):
    d = (a - b).reshape(-1, 3)
    if mask is not None:
        d = d[mask]
    return float(np.sqrt(np.mean(d * d)))


@pytest.mark.parametrize("scene,nx,ny,textured", [("cornell_box", 64, 64, None), ("random_balls", 60, 40, "none"),
                                                  ("textured", 48, 32, "some"), ("probe_textures", 48, 32, "some")])
def test_denoised_image_is_closer_to_the_converged_one(gpu, host_features, scene, nx, ny, textured):
    """16 spp plus features plus the filter against a 4096-spp render of the
    same scene with another seed: the canvas RMSE of the denoised image is
    below the raw 16-spp image's.  On the scenes with textures the RMSE over
    the pixels whose 16 samples all hit a textured primitive (a material whose
    texture is not a constant: tests/cpp/host_features.cpp) does not exceed the
    raw image's either: demodulation keeps the texture.  `textured` has image
    and checker-of-image textures, probe_textures a checker ground and marble
    spheres; random_balls has no textured primitive at all (its ground is a
    constant grey), which the test states, so that restriction is empty there."""
    spp, seed = 16, 21
    ds = gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny))
    try:
        r = gpu.render_denoised(ds, nx, ny, spp, DEPTH, seed, device_buffers=True)
        raw = ds.finalize_device(r["accum"], nx, ny, spp).cpu().numpy()
        den = r["canvas"].cpu().numpy()
        ref_acc, _ = ds.render_accumulate(nx, ny, 4096, DEPTH, seed + 1000)
        ref = gpu.finalize(ref_acc, nx, ny, 4096)
    finally:
        ds.close()
    assert np.isfinite(den).all()
    e_raw, e_den = rmse(raw, ref), rmse(den, ref)
    print(f"{scene} {nx}x{ny}: canvas RMSE raw {e_raw:.5f} denoised {e_den:.5f} ratio {e_den / e_raw:.4f}")
    assert e_den < e_raw
    if textured is None:
        return
    _, hits = host_features(scene, nx, ny, spp, seed)
    mask = hits == spp
    if textured == "none":
        assert not hits.any()
        return
    t_raw, t_den = rmse(raw, ref, mask), rmse(den, ref, mask)
    print(f"  textured pixels {int(mask.sum())} of {nx * ny}: RMSE raw {t_raw:.5f} denoised {t_den:.5f} "
          f"ratio {t_den / t_raw:.4f}")
    assert mask.mean() >= 0.1
    assert t_den <= t_raw


# ---- 14. the adaptive pairing --------------------------------------------------------------
@pytest.mark.parametrize("device_buffers", [False, True], ids=["host", "device"])
def test_adaptive_render_passes_its_counts_to_the_filter(gpu, device_buffers):
    nx, ny = 48, 32
    ds = gpu.DeviceScene(gpu.SceneDesc("cornell_box", nx / ny))
    try:
        r = gpu.render_adaptive(ds, nx, ny, 64, DEPTH, 3, target_rel=0.05, min_spp=8, device_buffers=device_buffers,
                                denoise=True)
        by_hand = ds.denoise(r["accum"], r["accum_sq"], r["features"], nx, ny, counts=r["counts"], feature_spp=8)
        feats, _ = ds.render_features(nx, ny, 64, 3, spp_count=8)
    finally:
        ds.close()
    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
    counts = host(r["counts"])
    assert counts.min() >= 8 and counts.max() > counts.min(), "the counts are not uniform"
    assert r["feature_spp"] == 8 and np.array_equal(host(r["features"]), feats)
    den = host(r["denoised"])
    assert np.isfinite(den).all() and np.array_equal(den, host(by_hand))
    want = gpu.denoise(host(r["accum"]), host(r["accum_sq"]), feats, nx, ny, counts=counts.astype(np.uint32),
                       feature_spp=8)
    assert np.array_equal(den, want)


# ---- 15. rtw_render --denoise ------------------------------------------------------------------
def test_cli_denoise(gpu, tmp_path):
    """--denoise writes a PPM and one Denoise: line, with plain, --noise-target
    and --adaptive renders; without the flag the PPM of ppm_cornell_48x48x8_d50
    is byte-identical to the golden."""
    base = [str(CLI), "--scene", "cornell_box", "--nx", "48", "--ny", "48", "--spp", "8", "--depth", "50", "--seed", "0"]
    plain = tmp_path / "plain.ppm"
    p = subprocess.run([*base, "--out", str(plain)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Denoise:" not in p.stdout, p.stdout + p.stderr
    assert plain.read_bytes() == (GOLD / "ppm_cornell_48x48x8_d50.ppm").read_bytes()
    for k, extra in enumerate(([], ["--denoise-iterations", "2"], ["--noise-target", "0.01", "--noise-batch", "4"],
                               ["--spp", "32", "--adaptive", "0.05", "--min-spp", "8"])):
        out = tmp_path / f"den{k}.ppm"
        p = subprocess.run([*base, *extra, "--denoise", "--out", str(out)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = [l for l in p.stdout.splitlines() if l.startswith("Denoise:")]
        assert len(lines) == 1 and re.fullmatch(r"Denoise: iterations \d+  [0-9.]+ ms", lines[0]), p.stdout
        assert int(lines[0].split()[2]) == (2 if k == 1 else 5)
        px = out.read_text().split()
        assert px[0] == "P3" and px[1:3] == ["48", "48"] and len(px) == 4 + 48 * 48 * 3
        assert out.read_bytes() != plain.read_bytes()
