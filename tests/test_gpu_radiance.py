"""Radiance queries on the GPU (include/rtw_radiance.h): rtw_trace_radiance
against the host classes ray by ray (tests/cpp/host_radiance.cpp), a render's
own paths bit for bit (rtw_camera_rays + the states it leaves), every execution
form to the same bits, keys instead of positions, sizes / pools / passes /
chunks, host and device buffers, the ADD semantics, the refusals that need a
device, and rtw_render --rays --radiance."""
import ctypes as C
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_denoise import FEATURE_CASES, _compile
from test_gpu_query import make_rays

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "raytracingweekend_amd"
CLI = PKG / "rtw_render"
N = 512
TOL = 1e-13  # the project's parity figure, relative to max(|value|, 1)
SPP, BEGIN, DEPTH, SEED, KEY = 3, 2, 50, 7, 123456

# (scene, bvh, normal)
HOST_CASES = [(c[0], c[1], False) for c in FEATURE_CASES] + [("ties", False, False), ("ties", True, False),
                                                             ("cornell_box", False, True)]
IDS = [f"{c[0]}-{'bvh' if c[1] else 'flat'}{'-normal' if c[2] else ''}" for c in HOST_CASES]


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


def scene_desc(gpu, scene, bvh, normal=False):
    from raytracingweekend_amd import _abi
    sd = gpu.SceneDesc(scene, 1.0, use_bvh=bvh)
    if normal:
        sd.desc.render_type = _abi.RTW_RENDER_NORMAL
    return sd


@pytest.fixture(scope="module")
def host_radiance(built, tmp_path_factory):
    exe = _compile("host_radiance.cpp", tmp_path_factory.mktemp("host_radiance") / "host_radiance")
    count = [0]

    def run(scene, rays, begin, count_, depth, seed, key, rng=None):
        """(per-ray sums (n, 3), traversals) of tests/cpp/host_radiance.cpp."""
        count[0] += 1
        base = exe.parent / f"case{count[0]}"
        rays.tofile(f"{base}.rays")
        if rng is not None:
            rng.tofile(f"{base}.rng")
        r = subprocess.run([str(exe), scene, f"{base}.rays", f"{base}.rng" if rng is not None else "-", str(begin),
                            str(count_), str(depth), str(seed), str(key), f"{base}.out"], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        n = len(rays)
        raw = np.fromfile(f"{base}.out", dtype=np.uint8)
        return raw[:n * 24].view(np.float64).reshape(n, 3).copy(), int(raw[n * 24:].view(np.uint64)[0])
    return run


def relerr(got, want):
    """Relative to max(|want|, 1); a NaN must be a NaN on both sides (then 0),
    an infinity the same infinity."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN channels differ"
    inf = np.isinf(want) | np.isinf(got)
    assert np.array_equal(got[inf], want[inf]), "infinite channels differ"
    ok = np.isfinite(want) & np.isfinite(got)
    e = np.zeros(want.shape)
    e[ok] = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1.0)
    return e


# ---- 1. against the host classes -------------------------------------------------------------
@pytest.mark.parametrize("scene,bvh,normal", HOST_CASES, ids=IDS)
def test_sums_match_the_host_classes(gpu, host_radiance, scene, bvh, normal):
    """512 rays, samples [2, 5) of each, depth 50, keys from 123456: every
    channel of every ray within 1e-13 relative to max(|v|, 1) of color() over
    the host classes under the same streams, no ray left out (a NaN channel is
    NaN on both sides), and stats.segments = the host's traversal count."""
    sd = scene_desc(gpu, scene, bvh, normal)
    rays, _ = make_rays(sd, n=N)
    want, traversals = host_radiance(("normal:" if normal else "") + scene, rays, BEGIN, SPP, DEPTH, SEED, KEY)
    ds = gpu.DeviceScene(sd)
    try:
        name = ds.query_radiance()
        got = ds.trace_radiance(rays, SPP, DEPTH, seed=SEED, spp_begin=BEGIN, first_key=KEY)
        st = ds.last_query_stats
    finally:
        ds.close()
    e = relerr(got, want)
    print(f"{scene} {'bvh' if bvh else 'flat'}{' normal' if normal else ''} {name}: max error {e.max():.3e} at ray "
          f"{int(np.argmax(e.max(axis=1)))}, NaN channels {int(np.isnan(want).sum())}, bit-identical "
          f"{np.array_equal(got, want, equal_nan=True)}, segments {st['segments']} / host {traversals}")
    assert got.shape == (N, 3) and want.any()
    assert e.max() <= TOL
    assert st["samples"] == N * SPP and st["segments"] == traversals
    assert st["launches_intersect"] >= 1 and st["ms_total"] > 0
    if normal:
        assert traversals == N * SPP


# ---- 2. a render's own paths, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("scene,bvh,nx,ny,spp", [("cornell_box", False, 16, 16, 3), ("random_balls", True, 24, 16, 2),
                                                  ("book2_final", True, 8, 8, 2)],
                         ids=["cornell_box", "random_balls-bvh", "book2_final-bvh"])
def test_a_renders_own_paths_bit_for_bit(gpu, scene, bvh, nx, ny, spp):
    """rtw_camera_rays' rays and the states it leaves, traced with one sample
    per ray and summed per pixel in sample order, are rtw_render_accumulate
    into zeros: np.array_equal, and equal segment totals."""
    ds = gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny, use_bvh=bvh))
    try:
        rays, rng = ds.camera_rays(nx, ny, spp, SEED)
        kept = rng.copy()
        sums = ds.trace_radiance(rays, 1, DEPTH, rng=rng)
        st = ds.last_query_stats
        name = ds.query_radiance()
        acc, st_r = ds.render_accumulate(nx, ny, spp, DEPTH, seed=SEED)
        kernel = ds.query()["kernel"]
    finally:
        ds.close()
    assert np.array_equal(rng, kept), "the states are read only"
    per_pixel = np.zeros((nx * ny, 3))
    for s in range(spp):
        per_pixel = per_pixel + sums[s * nx * ny:(s + 1) * nx * ny]
    print(f"{scene}: {name} against the render's {kernel}; segments {st['segments']} / {st_r['segments']}")
    assert name.startswith("k_persist") and acc.any()
    assert np.array_equal(per_pixel.ravel(), acc, equal_nan=True)
    assert st["segments"] == st_r["segments"] and st["samples"] == st_r["samples"] == nx * ny * spp


# ---- 3. every form gives the same bits ------------------------------------------------------------
FORM_SCENES = {"cornell_box": False, "random_balls": True}
# setting -> (environment, what query_radiance names for cornell_box flat, for random_balls + BVH)
FORMS = {"default": ({}, r"k_persist_sort<1136, 8, true>", r"k_persist<1154, 12, false, true>"),
         "wavefront": ({"RTW_MODE": "wavefront"}, r"k_regen_rays \+ k_segment<0, 8, true>",
                       r"k_regen_rays \+ (k_segment|k_intersect)<2[,>].*"),
         "split": ({"RTW_MODE": "wavefront", "RTW_SPLIT": "1"}, r"k_regen_rays \+ k_intersect<0>",
                   r"k_regen_rays \+ k_intersect<2>"),
         # k_persist without LDS stacks / k_persist_sort under a BVH have no ray row: the wavefront forms
         "sort0": ({"RTW_SORT": "0"}, r"k_regen_rays \+ k_segment<0, 8, true>", r"k_persist<1154, 12, false, true>"),
         "sort1": ({"RTW_SORT": "1"}, r"k_persist_sort<1136, 8, true>", r"k_regen_rays \+ (k_segment|k_intersect)<2[,>].*")}


@pytest.fixture(scope="module")
def form_reference(gpu, tmp_path_factory):
    """The rays of each form scene in a file, and the default selection's sums
    and segments, computed once in this process."""
    d = tmp_path_factory.mktemp("forms")
    ref = {}
    for scene, bvh in FORM_SCENES.items():
        sd = gpu.SceneDesc(scene, 1.0, use_bvh=bvh)
        rays, _ = make_rays(sd, n=N)
        np.save(d / f"{scene}.npy", rays)
        ds = gpu.DeviceScene(sd)
        try:
            sums = ds.trace_radiance(rays, SPP, DEPTH, seed=SEED, spp_begin=BEGIN, first_key=KEY)
            ref[scene] = (d / f"{scene}.npy", sums, ds.last_query_stats["segments"], ds.query_radiance())
        finally:
            ds.close()
    return ref


@pytest.mark.parametrize("setting", list(FORMS))
@pytest.mark.parametrize("scene", list(FORM_SCENES))
def test_every_form_gives_the_same_bits(gpu, form_reference, tmp_path, scene, setting):
    """The same call in a fresh process under the default selection,
    RTW_MODE=wavefront, RTW_SPLIT=1 and RTW_SORT=0 / 1 (read once per process):
    identical sums and segment counts, and query_radiance names the kernel the
    setting selects."""
    rays_file, want, segments, default_name = form_reference[scene]
    bvh = FORM_SCENES[scene]
    env, *names = FORMS[setting]
    out = tmp_path / "sums.npy"
    code = (f"import sys; sys.path.insert(0, {str(ROOT)!r}); import numpy as np; "
            f"from raytracingweekend_amd import render as r; "
            f"ds = r.DeviceScene(r.SceneDesc({scene!r}, 1.0, use_bvh={bvh})); "
            f"s = ds.trace_radiance(np.load({str(rays_file)!r}), {SPP}, {DEPTH}, seed={SEED}, spp_begin={BEGIN}, "
            f"first_key={KEY}); st = ds.last_query_stats; name = ds.query_radiance(); ds.close(); "
            f"np.save({str(out)!r}, s); print('SEGMENTS', st['segments']); print('KERNEL', name)")
    clean = {k: v for k, v in os.environ.items() if k not in ("RTW_MODE", "RTW_SPLIT", "RTW_SORT")}
    r = subprocess.run([sys.executable, "-c", code], env={**clean, **env}, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    name = r.stdout.split("KERNEL ")[-1].splitlines()[0]
    print(f"{scene} {setting}: {name}")
    assert re.fullmatch(names[1] if bvh else names[0], name), name
    if setting == "default":
        assert name == default_name
    assert int(r.stdout.split("SEGMENTS")[-1].split()[0]) == segments
    assert np.array_equal(np.load(out), want, equal_nan=True)


# ---- 4. keys, not positions -------------------------------------------------------------------------
@pytest.mark.parametrize("scene,bvh", [("cornell_box", False), ("book2_final", True)], ids=["cornell_box", "book2_final-bvh"])
def test_keys_not_positions(gpu, scene, bvh):
    """Rays [a, b) traced alone with first_key + a are rows [a, b) of the full
    call; rays permuted together with explicit states give permuted results."""
    sd = gpu.SceneDesc(scene, 1.0, use_bvh=bvh)
    rays, rng = make_rays(sd, n=N)
    ds = gpu.DeviceScene(sd)
    try:
        full = ds.trace_radiance(rays, SPP, DEPTH, seed=SEED, spp_begin=BEGIN, first_key=KEY)
        for a, b in ((0, 1), (100, 357), (N - 65, N)):
            part = ds.trace_radiance(np.ascontiguousarray(rays[a:b]), SPP, DEPTH, seed=SEED, spp_begin=BEGIN,
                                     first_key=KEY + a)
            assert np.array_equal(part, full[a:b], equal_nan=True), (a, b)
        moved = ds.trace_radiance(np.ascontiguousarray(rays[100:357]), SPP, DEPTH, seed=SEED, spp_begin=BEGIN,
                                  first_key=KEY)
        assert not np.array_equal(moved, full[100:357], equal_nan=True), "other keys are other paths"
        given = ds.trace_radiance(rays, 1, DEPTH, rng=rng)
        perm = np.random.default_rng(3).permutation(N)
        shuffled = ds.trace_radiance(np.ascontiguousarray(rays[perm]), 1, DEPTH, rng=np.ascontiguousarray(rng[perm]))
        assert np.array_equal(shuffled, given[perm], equal_nan=True) and given.any()
    finally:
        ds.close()


# ---- 5. sizes, pools, passes, chunks, buffers ---------------------------------------------------------
@pytest.mark.parametrize("scene,bvh", [("cornell_box", False), ("random_balls", True), ("nested", False)],
                         ids=["cornell_box", "random_balls-bvh", "nested"])
def test_sizes_pools_passes_and_buffers(gpu, monkeypatch, scene, bvh):
    """n = 0, 1, 63, 64, 65 are the first rows of the 1000-ray call; 256 paths
    in flight (the persistent queue drains across workgroups; under
    RTW_MODE=wavefront the pool refills many times), a budget of two samples per
    ray (passes of 2 + 2 + 1) and one below the ray count (several chunks, each
    with its own first key) change no bit; device tensors give the host
    buffers' bytes; a second call into the same sums doubles them."""
    import torch
    sd = gpu.SceneDesc(scene, 1.0, use_bvh=bvh)
    rays, _ = make_rays(sd, n=1000)
    spp = 5
    call = dict(seed=SEED, spp_begin=1, first_key=KEY)
    ds = gpu.DeviceScene(sd)
    try:
        base = ds.trace_radiance(rays, spp, DEPTH, **call)
        st = ds.last_query_stats
        persistent = ds.query_radiance().startswith("k_persist")
        assert st["samples"] == 5000 and base.any()
        if persistent:
            assert st["launches_intersect"] == 1
        for n in (0, 1, 63, 64, 65):
            part = ds.trace_radiance(np.ascontiguousarray(rays[:n]), spp, DEPTH, **call)
            assert part.shape == (n, 3) and np.array_equal(part, base[:n], equal_nan=True), n
            assert ds.last_query_stats["samples"] == n * spp
        small = ds.trace_radiance(rays, spp, DEPTH, wavefront_paths=256, **call)
        assert np.array_equal(small, base, equal_nan=True) and ds.last_query_stats["segments"] == st["segments"]
        # ADD semantics: into the first call's sums
        twice = ds.trace_radiance(rays, spp, DEPTH, out=base.copy(), **call)
        assert np.array_equal(twice, base + base, equal_nan=True)
        # device tensors
        dev = ds.trace_radiance(torch.from_numpy(rays).cuda(), spp, DEPTH, **call)
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), base, equal_nan=True)
        assert ds.last_query_stats["segments"] == st["segments"]
        # max_depth 0: nothing is added, the samples count
        zero = ds.trace_radiance(rays, spp, 0, out=base.copy(), **call)
        assert np.array_equal(zero, base, equal_nan=True)
        assert ds.last_query_stats["samples"] == 5000 and ds.last_query_stats["segments"] == 0
        # passes of 2 + 2 + 1 samples
        monkeypatch.setenv("RTW_PASS_SAMPLES", "2000")
        passes = ds.trace_radiance(rays, spp, DEPTH, **call)
        assert np.array_equal(passes, base, equal_nan=True) and ds.last_query_stats["segments"] == st["segments"]
        if persistent:
            assert ds.last_query_stats["launches_intersect"] == 3
        # chunks of 300, 300, 300 and 100 rays: a pass per sample, the last chunk passes of 3 + 2
        monkeypatch.setenv("RTW_PASS_SAMPLES", "300")
        chunks = ds.trace_radiance(rays, spp, DEPTH, **call)
        assert np.array_equal(chunks, base, equal_nan=True) and ds.last_query_stats["segments"] == st["segments"]
        if persistent:
            assert ds.last_query_stats["launches_intersect"] == 3 * 5 + 2
        dev = ds.trace_radiance(torch.from_numpy(rays).cuda(), spp, DEPTH, **call)
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), base, equal_nan=True)
        monkeypatch.delenv("RTW_PASS_SAMPLES")
        # the wavefront forms: the pool of 256 refills many times
        monkeypatch.setenv("RTW_MODE", "wavefront")
        assert ds.query_radiance().startswith("k_regen_rays + ")
        wave = ds.trace_radiance(rays, spp, DEPTH, wavefront_paths=256, **call)
        assert np.array_equal(wave, base, equal_nan=True) and ds.last_query_stats["segments"] == st["segments"]
        assert ds.last_query_stats["iterations"] >= 20
    finally:
        ds.close()


# ---- 6. refusals that need a device ------------------------------------------------------------------
def test_refusals_that_need_a_device(gpu):
    """A misaligned device pointer, host memory passed with on_device, the sums
    over the rays, fp32, a ray outside the shutter of a BVH scene with moving
    spheres (host and device buffers alike; flat, the same scene traces any
    time), and the strict build."""
    import torch
    from raytracingweekend_amd import _abi
    from raytracingweekend_amd._abi import RtwError
    L = _abi.lib()
    sd = gpu.SceneDesc("probe_motion", 1.0, use_bvh=True)
    rays, _ = make_rays(sd, n=64)
    ds = gpu.DeviceScene(sd)
    try:
        dev = torch.from_numpy(rays).cuda()
        out = torch.zeros((65, 3), dtype=torch.float64, device="cuda")
        states = torch.ones(65, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        prm = _abi.rtw_radiance_params(max_depth=5, spp_count=1, on_device=1)
        call = lambda r, o, g=None, p=prm, n=64: L.rtw_trace_radiance(ds.handle, C.c_void_p(r), n,
                                                                      C.c_void_p(g) if g else None, C.byref(p),
                                                                      C.c_void_p(o), None)
        assert call(dev.data_ptr(), out.data_ptr()) == 0
        assert call(dev.data_ptr(), out.data_ptr() + 8) == 0     # the sums need 8 bytes only
        assert call(dev.data_ptr(), out.data_ptr() + 4) == -1 and b"aligned" in L.rtw_last_error()
        assert call(dev.data_ptr() + 8, out.data_ptr(), n=63) == -1 and b"aligned" in L.rtw_last_error()
        assert call(dev.data_ptr(), out.data_ptr(), states.data_ptr() + 2) == -1 and b"aligned" in L.rtw_last_error()
        assert call(dev.data_ptr(), out.data_ptr(), states.data_ptr() + 4) == 0
        assert call(rays.ctypes.data, out.data_ptr()) == -1          # host memory passed as device memory
        host_sums = np.zeros((64, 3))
        assert call(dev.data_ptr(), host_sums.ctypes.data) == -1
        assert call(dev.data_ptr(), dev.data_ptr()) == -1 and b"overlap" in L.rtw_last_error()
        assert call(dev.data_ptr(), out.data_ptr(),
                    p=_abi.rtw_radiance_params(max_depth=5, spp_count=1, on_device=1, precision=1)) == -5
        # ... also where max_depth 0 leaves nothing to trace
        depth0 = _abi.rtw_radiance_params(max_depth=0, spp_count=1, on_device=1)
        assert call(rays.ctypes.data, out.data_ptr(), p=depth0) == -1
        assert call(dev.data_ptr(), host_sums.ctypes.data, p=depth0) == -1
        assert call(dev.data_ptr(), out.data_ptr(), p=depth0) == 0
        assert call(dev.data_ptr(), out.data_ptr(), n=0) == 0
        assert not host_sums.any()
        # the shutter: the spheres move, the BVH's boxes cover the desc camera's shutter only
        t0, t1 = sorted((sd.camera.time0, sd.camera.time1))
        assert t1 > t0
        late = rays.copy()
        late[17, 6] = t1 + 0.5
        for r in (late, torch.from_numpy(late).cuda()):
            with pytest.raises(RtwError, match="shutter"):
                ds.trace_radiance(r, 1, 5)
        nan = rays.copy()
        nan[3, 6] = np.nan
        with pytest.raises(RtwError, match="shutter"):
            ds.trace_radiance(nan, 1, 5)
        assert ds.trace_radiance(rays, 1, 5).shape == (64, 3)  # the handle still serves
        with pytest.raises(RtwError):
            ds.trace_radiance(rays, 1, 5, precision="fp32")
    finally:
        ds.close()
    ds = gpu.DeviceScene(gpu.SceneDesc("probe_motion", 1.0))
    try:
        assert ds.trace_radiance(late, 1, 5).shape == (64, 3)
    finally:
        ds.close()
    # the strict build has the symbols and refuses
    strict = _abi.load_library(PKG / "_build" / "librtw_strict.so")
    fake = C.c_int(0)
    assert strict.rtw_scene_query_radiance(C.byref(fake), C.create_string_buffer(128)) == -5
    prm = _abi.rtw_radiance_params(max_depth=5, spp_count=1)
    sums = np.zeros((64, 3))
    assert strict.rtw_trace_radiance(C.byref(fake), rays.ctypes.data_as(C.c_void_p), 64, None, C.byref(prm),
                                     sums.ctypes.data_as(C.c_void_p), None) == -5


# ---- 7. the CLI ------------------------------------------------------------------------------------------
def test_cli_round_trip(gpu, tmp_path):
    """rtw_render --rays / --radiance gives trace_radiance's bytes and one
    Radiance: line naming the kernel; with --rng, the given states' paths."""
    scene = "random_balls"
    sd = gpu.SceneDesc(scene, 1.0, use_bvh=True)
    rays, rng = make_rays(sd, n=500)
    ds = gpu.DeviceScene(sd)
    try:
        want = ds.trace_radiance(rays, 3, 20, seed=5)
        segments = ds.last_query_stats["segments"]
        given = ds.trace_radiance(rays, 1, 20, rng=rng)
        name = ds.query_radiance()
    finally:
        ds.close()
    rays.tofile(tmp_path / "rays.bin")
    rng.tofile(tmp_path / "rng.bin")
    base = [str(CLI), "--scene", scene, "--nx", "100", "--ny", "100", "--bvh", "--rays", str(tmp_path / "rays.bin")]
    p = subprocess.run([*base, "--radiance", str(tmp_path / "a.bin"), "--spp", "3", "--depth", "20", "--seed", "5"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith("Radiance:")]
    assert len(lines) == 1, p.stdout
    m = re.fullmatch(r"Radiance: (.+)  rays 500  samples 1500  segments (\d+)  [0-9.]+ ms", lines[0])
    assert m and m.group(1) == name and int(m.group(2)) == segments, lines[0]
    assert (tmp_path / "a.bin").read_bytes() == want.tobytes()
    p = subprocess.run([*base, "--radiance", str(tmp_path / "b.bin"), "--spp", "1", "--depth", "20", "--rng",
                        str(tmp_path / "rng.bin")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert (tmp_path / "b.bin").read_bytes() == given.tobytes()
    assert np.array_equal(np.fromfile(tmp_path / "rng.bin", dtype=np.uint32), rng)
    p = subprocess.run([*base, "--radiance", str(tmp_path / "c.bin"), "--spp", "2", "--rng", str(tmp_path / "rng.bin")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "spp_count" in p.stderr
