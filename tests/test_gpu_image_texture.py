"""Image textures on the GPU: the `textured` scene against the host classes'
render (tests/cpp/host_render.cpp; the C oracle knows no image texture), a
constant image against the constant texture, an emitting image against its
texels, the fp32 mode against the fp64 one, and the execution forms against
each other."""
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "raytracingweekend_amd"
TOL = 1e-4  # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


def _compile(src, exe):
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", f"-I{ROOT / 'include'}",
           f"-I{PKG / 'csrc' / 'host'}", f"-I{PKG / 'csrc' / 'host' / 'rtw'}", str(ROOT / "tests" / "cpp" / src),
           f"-L{PKG}", "-lrtw", f"-Wl,-rpath,{PKG}", "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def host_render(built, tmp_path_factory):
    return _compile("host_render.cpp", tmp_path_factory.mktemp("host_render") / "host_render")


@pytest.fixture(scope="module")
def image_scene(built, tmp_path_factory):
    return _compile("gpu_image_scene.cpp", tmp_path_factory.mktemp("gpu_image_scene") / "gpu_image_scene")


def finalize_np(sums, spp):
    return np.minimum(np.sqrt(sums / spp), 1.0)


# ------------------------------------------------------ fp64 vs the host classes
@pytest.fixture(scope="module")
def host_textured(host_render, tmp_path_factory):
    """The host classes' render of `textured` (flat list), once."""
    nx, ny, spp, depth, seed = 32, 24, 4, 10, 7
    out = tmp_path_factory.mktemp("textured") / "flat.bin"
    r = subprocess.run([str(host_render), "textured", str(nx), str(ny), str(spp), str(depth), str(seed), "flat",
                        str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    raw = out.read_bytes()
    sums = np.frombuffer(raw[:-8], dtype=np.float64).copy()
    sums.setflags(write=False)
    return (nx, ny, spp, depth, seed), sums, int(np.frombuffer(raw[-8:], dtype=np.uint64)[0])


@pytest.mark.parametrize("bvh", [False, True], ids=["flat", "bvh"])
def test_textured_matches_host_render(gpu, host_textured, bvh):
    """fp64 device render of `textured` (32x24, 4 spp, depth 10) against the
    host classes: equal traversal counts, canvas within 1e-4.

    Measured on one MI355X: max |canvas diff| 1.110e-16 flat and with BVHs;
    the largest relative difference of a pixel's radiance sum is 7.9e-16 (the
    bound below, 1e-9, tells ulps from a wrong texel)."""
    (nx, ny, spp, depth, seed), ref, seg = host_textured
    sd = gpu.SceneDesc("textured", nx / ny, use_bvh=bvh)
    ds = gpu.DeviceScene(sd)
    try:
        acc, st = ds.render_accumulate(nx, ny, spp, depth, seed=seed)
        info = ds.query()
    finally:
        ds.close()
    assert info["shade_mask"] & 32 and ", 63" in info["kernel"], info
    assert st["samples"] == nx * ny * spp
    assert st["segments"] == seg, "device-counted traversals differ from the host classes'"
    c_gpu, c_ref = finalize_np(acc, spp), finalize_np(ref, spp)
    assert np.all(np.isfinite(c_gpu))
    d = np.abs(c_gpu - c_ref)
    rel = np.abs(acc - ref) / np.maximum(np.abs(ref), 1e-300)
    print(f"textured bvh={bvh}: max |canvas diff| {d.max():.3e}, max relative sum diff {rel.max():.3e}, "
          f"kernel {info['kernel']}")
    assert d.max() <= TOL, f"max per-channel diff {d.max()} at {np.argmax(d)}"
    # a wrong texel (orientation, offsets) moves a pixel by far more than ulps
    assert rel.max() <= 1e-9, f"pixel channel {np.argmax(rel)} off by {rel.max()} relative: a finding, not ulps"
    # the image reaches the picture: the render differs from one channel to another
    img = acc.reshape(ny, nx, 3)
    assert np.abs(img[..., 0] - img[..., 2]).max() > 0.1


# ------------------------------------------------------ constant image == constant texture
@pytest.mark.parametrize("env", [{}, {"RTW_MODE": "wavefront"}, {"RTW_MODE": "wavefront", "RTW_SPLIT": "1"}],
                         ids=["persistent", "segment", "split"])
def test_constant_image_equals_constant_texture(image_scene, env):
    """A Cornell-like box with a 3x5 image of (186, 186, 186) texels on its
    white surfaces, and the same box with constant_texture(186 / 255.0): the
    radiance sums are bit-identical and the traversals equal, so the image
    path adds nothing but the lookup.  The constant scene's light list holds a
    sphere whose (never shaded) material carries the image, so both scenes run
    the same SF_IMAGE kernel (tests/cpp/gpu_image_scene.cpp)."""
    r = subprocess.run([str(image_scene), "identity"], capture_output=True, text=True, timeout=120,
                       env={**os.environ, **env})
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(ln.split(" ", 1) for ln in r.stdout.splitlines())
    assert out["kernel_image"] == out["kernel_const"], out
    assert ", 63" in out["kernel_image"] or out["kernel_image"].startswith("k_intersect"), out  # (k_shade<63> follows)
    assert out["shade_mask"].split()[0] == out["shade_mask"].split()[1] and int(out["shade_mask"].split()[0]) & 32
    sa, sb = out["segments"].split()
    assert sa == sb and int(sa) > 32 * 32 * 8
    assert out["identical"] == "1", out["maxdiff"]
    assert out["finite"] == "1" and float(out["total"]) > 0


def test_image_scene_without_a_persistent_kernel_falls_back(image_scene):
    """The same pair with a twelve-ball list that use_bvh turns into a group
    BVH (feature bit 4, F_GBVH): no persistent or fused kernel is instantiated for
    images with group BVHs, so the render takes the split k_intersect /
    k_shade pair -- and still looks the image up: bit-identical to the
    constant texture, whose value is far from the black a kernel without the
    lookup would return.  An fp32 render of it is refused
    (RTW_ERR_UNSUPPORTED), not rendered without the image."""
    r = subprocess.run([str(image_scene), "identity_gbvh"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(ln.split(" ", 1) for ln in r.stdout.splitlines())
    fa, fb = map(int, out["features"].split())
    assert fa == fb and fa & 4, out["features"]  # F_GBVH (and, with nine entries, a world BVH)
    assert out["kernel_image"] == out["kernel_const"] and out["kernel_image"].startswith("k_intersect<"), out
    assert int(out["shade_mask"].split()[0]) & 32 and int(out["shade_mask"].split()[1]) & 32
    sa, sb = out["segments"].split()
    assert sa == sb and int(sa) > 32 * 32 * 8
    assert out["identical"] == "1", out["maxdiff"]
    assert out["finite"] == "1" and float(out["total"]) > 0
    assert out["fp32_status"] == "-5"


# ------------------------------------------------------ an emitting image
def test_emitting_image_gives_its_texels(image_scene):
    """A pinhole camera looking straight at one diffuse_light xy_rect with a
    4x2 image (larger than the view, black background, 32x16, 8 spp, depth
    2): a pixel whose footprint lies inside one texel sums to exactly
    spp * texel / 255.0 per channel -- spp equal terms texel / 255.0 added in
    sample order, as the render loop adds them -- on the GPU and with the host
    classes.

    The footprint of pixel (i, j) on the rect's plane is the image of
    [i/nx, (i+1)/nx] x [j/ny, (j+1)/ny] under the camera's (affine, for a
    plane parallel to the image plane) map; it lies inside one texel when its
    four corners do, 1e-9 clear of every texel edge in (u, v) -- the rounding
    of camera::get_ray and of the rect's quotients is ~1e-16.  The rect is
    placed so that its three inner column edges and one row edge each fall
    inside one pixel column / row: 3 of 32 columns and 1 of 16 rows are left
    out (15 % of the pixels; the bound is 25 %)."""
    r = subprocess.run([str(image_scene), "emitter"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(ln.split(" ", 1) for ln in r.stdout.splitlines())
    nx, ny, spp = map(int, out["size"].split())
    vec = lambda k: np.array([float(x) for x in out[k].split()])  # noqa: E731
    origin, ll, hor, ver = vec("origin"), vec("lower_left"), vec("horizontal"), vec("vertical")
    x0, x1, y0, y1, k = vec("rect")
    img = [int(x) for x in out["image"].split()]
    inx, iny, texels = img[0], img[1], np.array(img[2:], dtype=np.float64).reshape(img[1], img[0], 3)
    gpu_sums = vec("gpu").reshape(ny, nx, 3)
    host_sums = vec("host").reshape(ny, nx, 3)
    assert int(out["segments"]) == nx * ny * spp  # a diffuse_light never scatters

    def texel_of(s, t):
        d = ll + s * hor + t * ver - origin
        p = origin + d * ((k - origin[2]) / d[2])
        u, v = (p[0] - x0) / (x1 - x0), (p[1] - y0) / (y1 - y0)
        fi, fj = u * inx, (1 - v) * iny - float(np.float32(0.001))
        eps = 1e-9
        if not (eps < u < 1 - eps and eps < v < 1 - eps):
            return None
        if min(fi - np.floor(fi), np.ceil(fi) - fi) < eps * inx or min(fj - np.floor(fj), np.ceil(fj) - fj) < eps * iny:
            return None
        return int(np.floor(fi)), int(np.floor(fj))

    used, seen = 0, set()
    for j in range(ny):
        for i in range(nx):
            corners = {texel_of((i + a) / nx, (j + b) / ny) for a in (0, 1) for b in (0, 1)}
            if len(corners) != 1 or None in corners:
                continue
            (ti, tj), = corners
            # the sum of spp equal samples in sample order (RayTracingWeekend.cpp:235-239);
            # it is spp * texel / 255.0 up to the roundings of that running sum
            x, want = texels[tj, ti] / 255.0, np.zeros(3)
            for _ in range(spp):
                want = want + x
            assert np.all(np.abs(want - spp * x) <= 4 * np.spacing(spp * x))
            assert np.array_equal(host_sums[j, i], want), ("host", i, j, host_sums[j, i], want)
            assert np.array_equal(gpu_sums[j, i], want), ("gpu", i, j, gpu_sums[j, i], want)
            used += 1
            seen.add((ti, tj))
    left_out = 1 - used / (nx * ny)
    print(f"emitter: {used} of {nx * ny} pixels checked, {left_out:.1%} left out, kernel {out['kernel']}")
    assert left_out <= 0.25
    assert seen == {(a, b) for a in range(inx) for b in range(iny)}  # every texel is seen, each its own colour
    assert len({tuple(t) for t in texels.reshape(-1, 3)}) == inx * iny
    # everywhere, edge pixels included, the GPU agrees with the host classes:
    # a rect's (u, v) are the host's own sums and quotients, bit for bit
    assert np.array_equal(gpu_sums, host_sums), f"max diff {np.abs(gpu_sums - host_sums).max()}"


# ------------------------------------------------------ fp32, statistically
def blocks(acc, nx, ny, spp, b=8):
    img = (acc / spp).reshape(ny, nx, 3)
    return img.reshape(ny // b, b, nx // b, b, 3).mean(axis=(1, 3)).reshape(-1, 3)


@pytest.mark.parametrize("bvh", [False, True], ids=["flat", "bvh"])
def test_fast_mode_is_statistically_the_fp64_render(gpu, bvh):
    """tests/test_gpu_fp32.py's comparison (its block-spread and bias
    formulas and constants) for `textured` at 64x48, 32 spp: 48 blocks x 3
    seeds = 144 block differences; the fp64 device render of seed 0 stands in
    for the oracle, which knows no image texture."""
    nx, ny, spp, depth = 64, 48, 32, 50
    sd = gpu.SceneDesc("textured", nx / ny, use_bvh=bvh)
    ds = gpu.DeviceScene(sd)
    try:
        ref, st_ref = ds.render_accumulate(nx, ny, spp, depth, seed=0)
        fast = [ds.render_accumulate(nx, ny, spp, depth, seed=k, precision="fp32") for k in (0, 1, 2)]
        other = [ds.render_accumulate(nx, ny, spp, depth, seed=k) for k in (1, 2, 3)]
        info = ds.query()
    finally:
        ds.close()
    seg_ref = st_ref["segments"]
    for acc, st in fast:
        assert st["samples"] == nx * ny * spp and np.all(np.isfinite(acc))
        assert st["bytes_intersect"] == 36 * st["segments"]
    assert info["kernel_fast"].startswith("k_fast<") and int(info["kernel_fast"][7:].split(",")[0]) & (1 << 13), info
    rb = blocks(ref, nx, ny, spp)
    d = np.concatenate([blocks(acc, nx, ny, spp) - rb for acc, _ in fast])
    e = np.concatenate([blocks(acc, nx, ny, spp) - rb for acc, _ in other])
    B = d.shape[0]
    assert B >= 96
    spread, base = float((d ** 2).mean()), float((e ** 2).mean())
    level = float(np.abs(ref).mean() / spp)
    bias = np.abs(d.mean(axis=0))
    print(f"textured fp32 bvh={bvh}: spread {spread:.3e} vs fp64 noise {base:.3e}; bias {bias} vs "
          f"{4 * np.sqrt(base / B) + 1e-3 * level:.3e}; kernel {info['kernel_fast']}")
    assert spread < 2.0 * base, f"block spread {spread:.3e} vs fp64-noise {base:.3e}"
    assert np.all(bias < 4 * np.sqrt(base / B) + 1e-3 * level), (bias, np.sqrt(base / B))
    seg32 = sum(st["segments"] for _, st in fast)
    seg64 = sum(st["segments"] for _, st in other)
    assert abs(seg32 / seg64 - 1) < 0.03
    assert abs(seg64 / 3 / seg_ref - 1) < 0.03


# ------------------------------------------------------ execution forms
def _render_in_child(env, scene, nx, ny, spp, depth, seed, bvh):
    with tempfile.TemporaryDirectory() as td:
        out = Path(td) / "acc.npy"
        code = (f"import sys; sys.path.insert(0, {str(ROOT)!r}); import numpy as np; "
                f"from raytracingweekend_amd import render as r; "
                f"ds = r.DeviceScene(r.SceneDesc({scene!r}, {nx}/{ny}, use_bvh={bvh})); "
                f"a, _ = ds.render_accumulate({nx}, {ny}, {spp}, {depth}, seed={seed}); ds.close(); "
                f"np.save({str(out)!r}, a)")
        subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, check=True, timeout=300)
        return np.load(out)


@pytest.mark.parametrize("bvh", [False, True], ids=["flat", "bvh"])
def test_execution_forms_agree_on_textured(gpu, monkeypatch, bvh):
    """As tests/test_gpu_parity.py test_execution_forms_agree: the persistent
    kernels (with and without regrouping, RTW_SORT), the wavefront's fused
    k_segment and its split pair render `textured` bit-identically -- no form
    drops the image."""
    nx, ny, spp, depth = 40, 30, 4, 50
    sd = gpu.SceneDesc("textured", nx / ny, use_bvh=bvh)
    ds = gpu.DeviceScene(sd)
    try:
        a, sa = ds.render_accumulate(nx, ny, spp, depth, seed=5)
        ka = ds.query()["kernel"]
        monkeypatch.setenv("RTW_MODE", "wavefront")
        b, sb = ds.render_accumulate(nx, ny, spp, depth, seed=5)
        kb = ds.query()["kernel"]
        monkeypatch.setenv("RTW_SPLIT", "1")
        c, sc = ds.render_accumulate(nx, ny, spp, depth, seed=5)
        kc = ds.query()["kernel"]
    finally:
        ds.close()
    assert ka.startswith("k_persist") and kb.startswith("k_segment") and kc.startswith("k_intersect"), (ka, kb, kc)
    assert sa["segments"] == sb["segments"] == sc["segments"]
    assert np.array_equal(a, b) and np.array_equal(a, c)
    assert np.all(np.isfinite(a)) and a.sum() > 0
    monkeypatch.delenv("RTW_MODE")
    monkeypatch.delenv("RTW_SPLIT")
    for sort in ("0", "1"):
        d = _render_in_child({"RTW_SORT": sort}, "textured", nx, ny, spp, depth, 5, bvh)
        assert np.array_equal(a, d), f"RTW_SORT={sort}"


def test_cli_renders_textured_with_a_loaded_image(gpu, tmp_path):
    """rtw_render --scene textured --image FILE.ppm: the first image comes
    from the loader; a different image gives a different picture."""
    from raytracingweekend_amd import build
    cli = build.CLI
    assert cli.exists()
    ppm = tmp_path / "in.ppm"
    ppm.write_bytes(b"P6\n2 2\n255\n" + bytes([255, 0, 0, 0, 255, 0, 0, 0, 255, 255, 255, 0]))
    outs = []
    for extra in ([], ["--image", str(ppm)]):
        out = tmp_path / f"o{len(outs)}.ppm"
        r = subprocess.run([str(cli), "--scene", "textured", "--nx", "32", "--ny", "24", "--spp", "4", "--depth", "10",
                            "--out", str(out), *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert out.read_text().startswith("P3\n32 24\n255\n")
        outs.append(out.read_text())
    assert outs[0] != outs[1]
