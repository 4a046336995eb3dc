"""The window rule of adaptive sampling on the GPU
(include/rtw_adaptive_window.h): the device select against the host select,
element for element, on the cases of tests/test_adaptive_window.py (which
checks the host select against the definition); the loop against
rtw_render_adaptive at radius 0 and against a replay through the host select at
radius 2; the strict build's refusal and the command-line tool.  All renders
use depth 50."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_adaptive import MAX_COUNT
from test_adaptive_window import HAND, RADII, SIZES, hand_cases, random_case
from test_noise import FLOOR, same_bits

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "raytracingweekend_amd" / "rtw_render"
DEPTH = 50


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


@pytest.fixture(scope="module")
def scene(gpu):
    """One handle for the selects: its scratch planes are reused, dirty, from
    case to case and grow with the images."""
    ds = gpu.DeviceScene(gpu.SceneDesc("cornell_box", 1.0))
    yield ds
    ds.close()


def to_device(s1, s2, counts):
    import torch
    return (torch.from_numpy(s1).to("cuda:0"), torch.from_numpy(s2).to("cuda:0"),
            torch.from_numpy(counts.astype(np.int32)).to("cuda:0"))


def device_list(ds, t, nx, ny, **kw):
    """The device select, twice on the same buffers: the same bits."""
    a = ds.select_active_window(*t, nx, ny, floor=FLOOR, **kw)
    assert a.is_cuda
    a = a.cpu().numpy().astype(np.uint32)
    b = ds.select_active_window(*t, nx, ny, floor=FLOOR, **kw).cpu().numpy().astype(np.uint32)
    assert np.array_equal(a, b), "the device select differs from call to call"
    return a


# (600, 500): the smallest size here whose 300 000 pixels exceed 1 024 blocks x 256,
# so that a block's chunk walks more than one tile
@pytest.mark.parametrize("nx,ny", SIZES + [(600, 500)])
def test_device_select_is_the_host_select(gpu, scene, nx, ny):
    c = random_case(nx, ny)
    if nx * ny > 1:
        assert 0.01 <= c["share"] <= 0.10, c["share"]
    t = to_device(c["s1"], c["s2"], c["counts"])
    for radius in RADII:
        for min_count in (0, 3):
            kw = dict(target_rel=c["target"], max_count=MAX_COUNT, min_count=min_count, radius=radius)
            host = gpu.select_active_window(c["s1"], c["s2"], c["counts"], nx, ny, floor=FLOOR, **kw)
            got = device_list(scene, t, nx, ny, **kw)
            assert got.size == host.size and np.array_equal(got, host), (nx, ny, radius, min_count, got.size, host.size)
    # radius 0 without min_count: the plain device select's list
    plain = scene.select_active(*t, nx, ny, target_rel=c["target"], max_count=MAX_COUNT, floor=FLOOR)
    got = device_list(scene, t, nx, ny, target_rel=c["target"], max_count=MAX_COUNT, min_count=0, radius=0)
    assert np.array_equal(got, plain.cpu().numpy().astype(np.uint32))


def test_hand_built_images(gpu, scene):
    nx, ny = HAND["nx"], HAND["ny"]
    for name, s1, s2, counts, want in hand_cases():
        got = device_list(scene, to_device(s1, s2, counts), nx, ny, target_rel=HAND["target"],
                          min_count=HAND["min_count"], max_count=HAND["max_count"], radius=HAND["radius"])
        assert np.array_equal(got, want), (name, got, want)


def test_scratch_grows_and_is_reused(gpu):
    """A large image after a small one on a fresh handle, then the small one
    again in the large one's planes."""
    ds = gpu.DeviceScene(gpu.SceneDesc("cornell_box", 1.0))
    try:
        for nx, ny in ((5, 3), (600, 500), (65, 4), (5, 3)):
            c = random_case(nx, ny)
            kw = dict(target_rel=c["target"], max_count=MAX_COUNT, min_count=0, radius=2)
            host = gpu.select_active_window(c["s1"], c["s2"], c["counts"], nx, ny, floor=FLOOR, **kw)
            got = device_list(ds, to_device(c["s1"], c["s2"], c["counts"]), nx, ny, **kw)
            assert np.array_equal(got, host), (nx, ny)
    finally:
        ds.close()


def test_device_refusals(gpu, scene):
    from raytracingweekend_amd import _abi
    c = random_case(5, 3)
    t = to_device(c["s1"], c["s2"], c["counts"])
    for kw, word in ((dict(radius=-1), "radius"), (dict(radius=17), "radius"), (dict(min_count=9, max_count=8), "min_count"),
                     (dict(target_rel=-1.0), "target_rel"), (dict(floor=0.0), "floor")):
        args = {**dict(target_rel=0.1, max_count=MAX_COUNT, min_count=0, radius=1, floor=FLOOR), **kw}
        with pytest.raises(_abi.RtwError, match=word) as e:
            scene.select_active_window(*t, 5, 3, **args)
        assert "(-1)" in str(e.value)
    # host buffers are not the handle's device's
    n = C.c_uint64()
    out = np.zeros(15, np.uint32)
    ptr = [x.ctypes.data_as(C.c_void_p) for x in (c["s1"], c["s2"], c["counts"], out)]
    rc = _abi.lib().rtw_adaptive_select_window_device(scene.handle, ptr[0], ptr[1], ptr[2], 5, 3, FLOOR, 0.1, 0, 8, 1,
                                                      ptr[3], C.byref(n))
    assert rc == -1 and b"not device" in _abi.lib().rtw_last_error()


# ---- the loop -----------------------------------------------------------------------
LOOP = dict(nx=48, ny=32, seed=7, min_spp=4, max_spp=32, batch=0)
COUNTERS = ("samples", "segments", "iterations", "launches_intersect")


def window_loop(gpu, ds, radius, target, precision="fp64", device_buffers=False):
    """rtw_render_adaptive_window through the C ABI, radius 0 included (which
    render.render_adaptive hands to rtw_render_adaptive)."""
    from raytracingweekend_amd import _abi
    nx, ny = LOOP["nx"], LOOP["ny"]
    ap = _abi.rtw_adaptive_params(target_rel=target, floor=FLOOR, min_spp=LOOP["min_spp"], max_spp=LOOP["max_spp"],
                                  batch=LOOP["batch"])
    if device_buffers:
        import torch
        bufs = [torch.full((nx * ny * 3,), 0.5, dtype=torch.float64, device="cuda:0") for _ in range(2)]
        bufs.append(torch.full((nx * ny,), 5, dtype=torch.int32, device="cuda:0"))
        torch.cuda.synchronize()
        ptrs = [C.c_void_p(t.data_ptr()) for t in bufs]
    else:
        # (prefilled: the loop overwrites, it does not add)
        bufs = [np.full(nx * ny * 3, 0.5), np.full(nx * ny * 3, 0.5), np.full(nx * ny, 5, dtype=np.uint32)]
        ptrs = [a.ctypes.data_as(C.c_void_p) for a in bufs]
    prm = _abi.rtw_render_params(nx=nx, ny=ny, spp=LOOP["max_spp"], max_depth=DEPTH, seed=LOOP["seed"], row_step=1,
                                 accum_on_device=int(device_buffers), precision=_abi.PRECISIONS[precision])
    res, st = _abi.rtw_adaptive_result(), _abi.rtw_stats()
    _abi.check(_abi.lib().rtw_render_adaptive_window(ds.handle, C.byref(ds.scene.camera), C.byref(prm), C.byref(ap),
                                                     radius, *ptrs, C.byref(res), C.byref(st)),
               "rtw_render_adaptive_window")
    if device_buffers:
        bufs = [t.cpu().numpy() for t in bufs]
        bufs[2] = bufs[2].astype(np.uint32)
    return dict(accum=bufs[0], accum_sq=bufs[1], counts=bufs[2], rounds=res.rounds, samples=res.samples,
                pixels_at_max=res.pixels_at_max, summary=res.final.as_dict(), stats=st.as_dict())


_replays = {}


def replay(gpu, name, radius=2):
    """The loop in Python: the whole image's moments of [0, min_spp), then per
    round the HOST select_active_window with min_count = done and the active
    render.  The target is the quantile of the first round's rel values whose
    round-1 list is nearest to half the image (the median itself would list
    every pixel: a radius-2 window of 25 pixels holds a source almost surely)."""
    if name in _replays:
        return _replays[name]
    from test_adaptive import rel_np
    nx, ny, seed = LOOP["nx"], LOOP["ny"], LOOP["seed"]
    npix = nx * ny
    ds = gpu.DeviceScene(gpu.SceneDesc(name, nx / ny))
    try:
        a, q = np.zeros(npix * 3), np.zeros(npix * 3)
        counts = np.zeros(npix, dtype=np.uint32)
        ds.render_moments(nx, ny, LOOP["max_spp"], DEPTH, seed, spp_begin=0, spp_count=LOOP["min_spp"], accum=a,
                          accum_sq=q)
        counts[:] = LOOP["min_spp"]
        rel, _, fin = rel_np(a, q, counts)
        assert fin.all()
        kw = dict(max_count=LOOP["max_spp"], radius=radius, floor=FLOOR)
        shares = {}
        for quantile in (0.5, 0.75, 0.9, 0.95, 0.98, 0.99, 0.995):
            t = float(np.quantile(rel, quantile))
            shares[t] = gpu.select_active_window(a, q, counts, nx, ny, target_rel=t, min_count=LOOP["min_spp"],
                                                 **kw).size / npix
        target = min(shares, key=lambda t: abs(shares[t] - 0.5))
        listed, rounds, done = [npix], 1, LOOP["min_spp"]
        for begin, count in gpu.adaptive_schedule(LOOP["min_spp"], LOOP["max_spp"], LOOP["batch"])[1:]:
            assert begin == done
            act = gpu.select_active_window(a, q, counts, nx, ny, target_rel=target, min_count=done, **kw)
            if act.size == 0:
                break
            ds.render_active(nx, ny, LOOP["max_spp"], DEPTH, seed, active=act, accum=a, accum_sq=q, counts=counts,
                             spp_begin=begin, spp_count=count)
            listed.append(int(act.size))
            rounds += 1
            done += count
    finally:
        ds.close()
    print(f"{name}: target {target:.5f}, round-1 shares by target {shares}, pixels listed per round {listed}")
    _replays[name] = dict(accum=a, accum_sq=q, counts=counts, target=target, rounds=rounds, listed=listed)
    return _replays[name]


@pytest.mark.parametrize("name", ["cornell_box", "random_balls"])
@pytest.mark.parametrize("device_buffers", [False, True])
def test_the_loop(gpu, name, device_buffers):
    nx, ny = LOOP["nx"], LOOP["ny"]
    npix = nx * ny
    ref = replay(gpu, name)
    # some later round lists some but not all pixels: otherwise the comparisons prove nothing
    assert any(0 < n < npix for n in ref["listed"][1:]), ref["listed"]
    ds = gpu.DeviceScene(gpu.SceneDesc(name, nx / ny))
    try:
        plain = gpu.render_adaptive(ds, nx, ny, LOOP["max_spp"], DEPTH, LOOP["seed"], target_rel=ref["target"],
                                    min_spp=LOOP["min_spp"], batch=LOOP["batch"], floor=FLOOR,
                                    device_buffers=device_buffers)
        r0 = window_loop(gpu, ds, 0, ref["target"], device_buffers=device_buffers)
        r2 = window_loop(gpu, ds, 2, ref["target"], device_buffers=device_buffers)
        via_python = gpu.render_adaptive(ds, nx, ny, LOOP["max_spp"], DEPTH, LOOP["seed"], target_rel=ref["target"],
                                         min_spp=LOOP["min_spp"], batch=LOOP["batch"], floor=FLOOR,
                                         device_buffers=device_buffers, window=2)
    finally:
        ds.close()
    if device_buffers:
        for r in (plain, via_python):
            r["accum"], r["accum_sq"] = r["accum"].cpu().numpy(), r["accum_sq"].cpu().numpy()
            r["counts"] = r["counts"].cpu().numpy().astype(np.uint32)
    # radius 0: rtw_render_adaptive bit for bit
    assert same_bits(r0["accum"], plain["accum"]) and same_bits(r0["accum_sq"], plain["accum_sq"])
    assert np.array_equal(r0["counts"], plain["counts"]) and 0 < plain["samples"] < npix * LOOP["max_spp"]
    for k in ("rounds", "samples", "pixels_at_max", "summary"):
        assert r0[k] == plain[k], k
    for k in COUNTERS:
        assert r0["stats"][k] == plain["stats"][k], k
    # radius 2: the replay through the host select
    assert same_bits(r2["accum"], ref["accum"]) and same_bits(r2["accum_sq"], ref["accum_sq"])
    assert np.array_equal(r2["counts"], ref["counts"])
    assert r2["rounds"] == ref["rounds"] and r2["samples"] == int(ref["counts"].sum()) == r2["stats"]["samples"]
    assert r2["pixels_at_max"] == int((ref["counts"] == LOOP["max_spp"]).sum())
    assert [int((ref["counts"] > b).sum()) for b, _ in gpu.adaptive_schedule(LOOP["min_spp"], LOOP["max_spp"])[1:r2["rounds"]]] \
        == ref["listed"][1:]
    # ... which render.render_adaptive(window=2) returns too
    assert same_bits(via_python["accum"], r2["accum"]) and np.array_equal(via_python["counts"], r2["counts"])
    assert via_python["rounds"] == r2["rounds"] and via_python["samples"] == r2["samples"]
    # every pixel takes at least the samples it takes under radius 0, some take more
    assert (r2["counts"] >= r0["counts"]).all() and (r2["counts"] > r0["counts"]).any()


def test_the_loop_fp32_radius_0(gpu):
    nx, ny = LOOP["nx"], LOOP["ny"]
    target = replay(gpu, "cornell_box")["target"]
    ds = gpu.DeviceScene(gpu.SceneDesc("cornell_box", nx / ny))
    try:
        plain = gpu.render_adaptive(ds, nx, ny, LOOP["max_spp"], DEPTH, LOOP["seed"], target_rel=target,
                                    min_spp=LOOP["min_spp"], batch=LOOP["batch"], floor=FLOOR, precision="fp32")
        r0 = window_loop(gpu, ds, 0, target, precision="fp32")
        r2 = window_loop(gpu, ds, 2, target, precision="fp32")
    finally:
        ds.close()
    assert same_bits(r0["accum"], plain["accum"]) and same_bits(r0["accum_sq"], plain["accum_sq"])
    assert np.array_equal(r0["counts"], plain["counts"])
    assert 0 < plain["samples"] < nx * ny * LOOP["max_spp"] and len(set(plain["counts"].tolist())) > 1
    for k in ("rounds", "samples", "pixels_at_max", "summary"):
        assert r0[k] == plain[k], k
    for k in COUNTERS:
        assert r0["stats"][k] == plain["stats"][k], k
    assert (r2["counts"] >= r0["counts"]).all()


def test_strict_build_refuses_the_loop(gpu):
    from raytracingweekend_amd import _abi, build
    L = _abi.load_library(build.STRICT_LIB)
    nx, ny = 8, 8
    d = C.POINTER(_abi.rtw_scene_desc)()
    _abi.check(L.rtw_scene_builtin(b"cornell_box", 1.0, 0, C.byref(d)), "strict builtin")
    h = C.c_void_p()
    try:
        assert L.rtw_scene_upload(0, d, C.byref(h)) == 0, L.rtw_last_error()
        bufs = [np.full(nx * ny * 3, 0.5), np.full(nx * ny * 3, 0.5), np.full(nx * ny, 5, dtype=np.uint32)]
        ptrs = [a.ctypes.data_as(C.c_void_p) for a in bufs]
        prm = _abi.rtw_render_params(nx=nx, ny=ny, spp=8, max_depth=DEPTH, seed=1, row_step=1)
        ap = _abi.rtw_adaptive_params(target_rel=0.1, floor=FLOOR, min_spp=4, max_spp=8, batch=0)
        for radius in (0, 2):
            rc = L.rtw_render_adaptive_window(h, C.byref(d.contents.camera), C.byref(prm), C.byref(ap), radius, *ptrs,
                                              None, None)
            assert rc == -5 and b"rtw_render_adaptive_window" in L.rtw_last_error(), (rc, L.rtw_last_error())
        assert (bufs[0] == 0.5).all() and (bufs[1] == 0.5).all() and (bufs[2] == 5).all()
    finally:
        if h:
            L.rtw_scene_free(h)
        L.rtw_scene_desc_free(d)


def test_cli(gpu, tmp_path):
    nx, ny = LOOP["nx"], LOOP["ny"]
    ref = replay(gpu, "random_balls")
    out = tmp_path / "w.ppm"
    base = [str(CLI), "--scene", "random_balls", "--nx", str(nx), "--ny", str(ny), "--spp", str(LOOP["max_spp"]),
            "--depth", str(DEPTH), "--seed", str(LOOP["seed"]), "--min-spp", str(LOOP["min_spp"]), "--noise-floor",
            repr(FLOOR), "--out", str(out)]
    p = subprocess.run(base + ["--adaptive", repr(ref["target"]), "--adaptive-window", "2"], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"^Adaptive: rounds (\d+)  samples (\d+) of (\d+)  mean_rel (\S+)  max_rel (\S+)  at_max (\d+)"
                  r"  window 2$", p.stdout, re.M)
    assert m, p.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(6))) == \
        (ref["rounds"], int(ref["counts"].sum()), nx * ny * LOOP["max_spp"], int((ref["counts"] == LOOP["max_spp"]).sum()))
    canvas = gpu.finalize_counts(ref["accum"], ref["counts"], nx, ny)
    want = (np.float64(np.float32(255.99)) * canvas).astype(np.int64).reshape(ny, nx, 3)[::-1].reshape(-1)
    tok = out.read_text().split()
    assert tok[:4] == ["P3", str(nx), str(ny), "255"]
    got = np.array(tok[4:], dtype=np.int64)
    assert got.size == want.size and (got != want).sum() <= max(1, want.size // 10000)
    # radius 0 does not name a window; the option alone is a usage error
    p = subprocess.run(base + ["--adaptive", repr(ref["target"]), "--adaptive-window", "0"], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0 and re.search(r"^Adaptive: .* at_max \d+$", p.stdout, re.M), p.stdout + p.stderr
    p = subprocess.run(base + ["--adaptive-window", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--adaptive-window needs --adaptive" in p.stderr, p.stdout + p.stderr
