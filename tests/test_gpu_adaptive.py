"""Adaptive per-pixel sampling on the GPU (include/rtw_adaptive.h).

The reference throughout is render_moments of the same sample range on the
whole image -- the code path that existed before the active-pixel kernels.  An
active render must give, on the listed pixels, exactly those bits
(np.array_equal), leave every other entry of the buffers untouched (0.5
prefill, as test_gpu_noise.test_rows_ranges_and_add_semantics) and count
exactly.  All renders use depth 50 or less."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_adaptive import MAX_COUNT, active_np, moments, rel_np
from test_noise import FLOOR, same_bits

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "raytracingweekend_amd" / "rtw_render"
DEPTH = 50
F_ACTIVE = 512


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


def template_f(name):
    """The first template argument (the feature bits) of a kernel name."""
    return int(re.search(r"<(\d+)", name).group(1))


def reference(ds, nx, ny, spp, seed, begin, count, precision, fill=0.5):
    """The whole image's render_moments of [begin, begin + count) into buffers
    prefilled with `fill`."""
    a, q = np.full(nx * ny * 3, fill), np.full(nx * ny * 3, fill)
    _, _, st = ds.render_moments(nx, ny, spp, DEPTH, seed, spp_begin=begin, spp_count=count, accum=a, accum_sq=q,
                                 precision=precision)
    return a, q, st


def check_active(ds, nx, ny, spp, seed, begin, count, precision, listed, ref, what, **kw):
    """One active render of `listed` into 0.5 / 5 prefilled buffers against the
    reference; returns its stats."""
    ref_a, ref_q, _ = ref
    a, q = np.full(nx * ny * 3, 0.5), np.full(nx * ny * 3, 0.5)
    counts = np.full(nx * ny, 5, dtype=np.uint32)
    st = ds.render_active(nx, ny, spp, DEPTH, seed, active=listed, accum=a, accum_sq=q, counts=counts, spp_begin=begin,
                          spp_count=count, precision=precision, **kw)
    on = np.zeros(nx * ny, dtype=bool)
    on[listed] = True
    on3 = np.repeat(on, 3)
    assert np.array_equal(a[on3], ref_a[on3]), f"{what}: accum differs on the listed pixels"
    assert np.array_equal(q[on3], ref_q[on3]), f"{what}: accum_sq differs on the listed pixels"
    assert (a[~on3] == 0.5).all() and (q[~on3] == 0.5).all(), f"{what}: an unlisted pixel was written"
    assert np.array_equal(counts, np.where(on, 5 + count, 5)), f"{what}: counts"
    assert st["samples"] == listed.size * count, what
    return st


def lists_64x48():
    nx, ny = 64, 48
    npix = nx * ny
    rng = np.random.default_rng(5)
    ij = np.arange(npix)
    out = {"last pixel": np.array([npix - 1]), "one row": np.arange(17 * nx, 18 * nx),
           "checkerboard": ij[((ij // nx) + (ij % nx)) % 2 == 0], "all": ij}
    for n in (63, 65, 1025):
        out[f"random {n}"] = np.sort(rng.choice(npix, n, replace=False))
    return {k: v.astype(np.uint32) for k, v in out.items()}


@pytest.mark.parametrize("scene,bvh,precision,family", [
    ("cornell_box", False, "fp64", "k_persist_sort<"), ("cornell_box", False, "fp32", "k_fast_sort<"),
    ("random_balls", True, "fp64", "k_persist<"), ("random_balls", True, "fp32", "k_fast<")])
def test_queue_edges(gpu, scene, bvh, precision, family):
    """List lengths 1, 63, 64, 65, 1 025, 1 536 and all 3 072 pixels of a 64x48
    image, 1 and 8 samples from sample 3: where the sample queue's
    reservations and the reduction's grid can go wrong."""
    nx, ny, spp, seed = 64, 48, 16, 3
    ds = gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny, use_bvh=bvh))
    try:
        name = ds.query_active(precision)
        assert name.startswith(family) and template_f(name) & F_ACTIVE, name
        whole = ds.query()["kernel" if precision == "fp64" else "kernel_fast"]
        assert not template_f(whole) & F_ACTIVE and template_f(name) == template_f(whole) | F_ACTIVE, (name, whole)
        for count in (1, 8):
            ref = reference(ds, nx, ny, spp, seed, 3, count, precision)
            for what, listed in lists_64x48().items():
                st = check_active(ds, nx, ny, spp, seed, 3, count, precision, listed, ref, f"{what} x{count}")
                if what == "all":
                    assert st["segments"] == ref[2]["segments"]
        # an empty list is a no-op
        a = np.full(nx * ny * 3, 0.5)
        st = ds.render_active(nx, ny, spp, DEPTH, seed, active=np.zeros(0, np.uint32), accum=a, precision=precision)
        assert st["samples"] == 0 and (a == 0.5).all()
    finally:
        ds.close()


def test_disjoint_lists_and_refusals(gpu):
    from raytracingweekend_amd import _abi
    nx, ny, spp, seed = 64, 48, 16, 3
    lists = lists_64x48()
    A = lists["checkerboard"]
    B = np.setdiff1d(lists["all"], A).astype(np.uint32)
    ds = gpu.DeviceScene(gpu.SceneDesc("cornell_box", nx / ny))
    try:
        ref = reference(ds, nx, ny, spp, seed, 3, 8, "fp64")
        sa = check_active(ds, nx, ny, spp, seed, 3, 8, "fp64", A, ref, "A")
        sb = check_active(ds, nx, ny, spp, seed, 3, 8, "fp64", B, ref, "B")
        assert sa["segments"] + sb["segments"] == ref[2]["segments"]
        assert sa["samples"] == A.size * 8 and sb["samples"] == B.size * 8
        # optional buffers: no accum_sq, no counts
        a = np.full(nx * ny * 3, 0.5)
        ds.render_active(nx, ny, spp, DEPTH, seed, active=A, accum=a, spp_begin=3, spp_count=8)
        on3 = np.repeat(np.isin(lists["all"], A), 3)
        assert np.array_equal(a[on3], ref[0][on3]) and (a[~on3] == 0.5).all()
        # no depth: no radiance, the samples still count
        c = np.full(nx * ny, 5, dtype=np.uint32)
        ds.render_active(nx, ny, spp, 0, seed, active=A, accum=a, counts=c, spp_begin=3, spp_count=8)
        assert np.array_equal(a[on3], ref[0][on3]) and np.array_equal(c, np.where(on3[::3], 13, 5))
        # refusals, before any launch: the buffers stay as they are
        a, q = np.full(nx * ny * 3, 0.5), np.full(nx * ny * 3, 0.5)
        c = np.full(nx * ny, 5, dtype=np.uint32)
        kw = dict(accum=a, accum_sq=q, counts=c, spp_begin=3, spp_count=8)
        for bad, word in ((dict(active=A, row_begin=1), "row_begin"), (dict(active=A, row_step=2), "row_begin"),
                          (dict(active=np.array([5, 4], np.uint32)), "ascending"),
                          (dict(active=np.array([4, 4], np.uint32)), "ascending"),
                          (dict(active=np.array([4, nx * ny], np.uint32)), "pixels"),
                          (dict(active=c[:16]), "overlap")):
            with pytest.raises(_abi.RtwError, match=word) as e:
                ds.render_active(nx, ny, spp, DEPTH, seed, **{**kw, **bad})
            assert "(-1)" in str(e.value)
        assert (a == 0.5).all() and (q == 0.5).all() and (c == 5).all()
    finally:
        ds.close()


def test_book2_and_the_wavefront_route(gpu):
    from raytracingweekend_amd import _abi
    nx, ny, spp, seed = 24, 24, 2, 7
    rng = np.random.default_rng(1)
    listed = np.sort(rng.choice(nx * ny, nx * ny // 2, replace=False)).astype(np.uint32)
    # (scene, BVHs, precision, what the active kernel's name must be)
    cases = [("book2_final", True, "fp64", lambda n: n.startswith("k_persist<") and template_f(n) & F_ACTIVE),
             ("book2_final", True, "fp32", lambda n: n.startswith("k_fast<") and template_f(n) & F_ACTIVE),
             ("nested", False, "fp64", lambda n: n.startswith("k_regen_active + ")),
             ("nested", False, "fp32", lambda n: n.startswith("k_fast<") and template_f(n) & F_ACTIVE),
             ("textured", False, "fp64", lambda n: n.startswith("k_regen_active + "))]
    for scene, bvh, precision, named in cases:
        ds = gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny, use_bvh=bvh))
        try:
            name = ds.query_active(precision)
            assert named(name), (scene, precision, name)
            ref = reference(ds, nx, ny, spp, seed, 0, 2, precision)
            check_active(ds, nx, ny, spp, seed, 0, 2, precision, listed, ref, f"{scene} {precision}")
        finally:
            ds.close()
    ds = gpu.DeviceScene(gpu.SceneDesc("textured", 1.0))
    try:
        a = np.full(nx * ny * 3, 0.5)
        with pytest.raises(_abi.RtwError, match="image textures") as e:
            ds.render_active(nx, ny, spp, DEPTH, seed, active=listed, accum=a, precision="fp32")
        assert "(-5)" in str(e.value) and (a == 0.5).all()
        with pytest.raises(_abi.RtwError, match="image textures"):
            ds.query_active("fp32")
    finally:
        ds.close()


@pytest.mark.parametrize("scene,bvh,general", [
    ("probe_textures", False, 516),  # a list scene: the whole image regroups (k_fast_sort<0, l>)
    ("probe_textures", True, 518),   # a world BVH with the marble texture (k_fast<2, l>)
    ("probe_medium", False, 517)])   # media without group BVHs (k_fast_sort<1, l>)
def test_general_fp32_rows(gpu, scene, bvh, general):
    """A scene without an fp32 row of its own renders a list with the general
    k_fast<.., false> of its traversal walk -- another kernel than the whole
    image's -- to the whole image's bits."""
    nx, ny, spp, seed = 24, 24, 2, 7
    listed = np.sort(np.random.default_rng(2).choice(nx * ny, nx * ny // 2, replace=False)).astype(np.uint32)
    ds = gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny, use_bvh=bvh))
    try:
        name, whole = ds.query_active("fp32"), ds.query()["kernel_fast"]
        assert name.startswith("k_fast<") and template_f(name) == general, (name, whole)
        assert (whole.split("<")[0], template_f(whole) | F_ACTIVE) != ("k_fast", general), (name, whole)
        ref = reference(ds, nx, ny, spp, seed, 0, 2, "fp32")
        check_active(ds, nx, ny, spp, seed, 0, 2, "fp32", listed, ref, f"{scene} fp32")
    finally:
        ds.close()


def test_passes_and_forms(gpu, monkeypatch):
    nx, ny, spp, seed = 64, 48, 16, 3
    listed = lists_64x48()["random 1025"]
    ds = gpu.DeviceScene(gpu.SceneDesc("cornell_box", nx / ny))
    try:
        for precision in ("fp64", "fp32"):
            ref = reference(ds, nx, ny, spp, seed, 3, 8, precision)
            one = check_active(ds, nx, ny, spp, seed, 3, 8, precision, listed, ref, "one pass")
            assert one["launches_intersect"] == 1
            monkeypatch.setenv("RTW_PASS_SAMPLES", str(3 * listed.size))  # passes of 3 + 3 + 2 samples
            st = check_active(ds, nx, ny, spp, seed, 3, 8, precision, listed, ref, "3 + 3 + 2")
            assert st["launches_intersect"] == 3 and st["segments"] == one["segments"]
            monkeypatch.delenv("RTW_PASS_SAMPLES")
        ref = reference(ds, nx, ny, spp, seed, 3, 8, "fp64")
        monkeypatch.setenv("RTW_MODE", "wavefront")
        assert ds.query_active("fp64").startswith("k_regen_active + k_segment<")
        check_active(ds, nx, ny, spp, seed, 3, 8, "fp64", listed, ref, "wavefront", wavefront_paths=1000)
        monkeypatch.setenv("RTW_SPLIT", "1")
        assert ds.query_active("fp64").startswith("k_regen_active + k_intersect<")
        check_active(ds, nx, ny, spp, seed, 3, 8, "fp64", listed, ref, "split", wavefront_paths=1000)
        monkeypatch.setenv("RTW_PASS_SAMPLES", str(3 * listed.size))
        st = check_active(ds, nx, ny, spp, seed, 3, 8, "fp64", listed, ref, "split, 3 + 3 + 2", wavefront_paths=1000)
    finally:
        ds.close()


def test_device_buffers(gpu):
    import torch
    from raytracingweekend_amd import _abi
    nx, ny, spp, seed = 64, 48, 16, 3
    listed = lists_64x48()["random 1025"]
    sd = gpu.SceneDesc("cornell_box", nx / ny)
    ds = gpu.DeviceScene(sd)
    try:
        ref_a, ref_q, _ = reference(ds, nx, ny, spp, seed, 3, 8, "fp64")
        dev = "cuda:0"
        ta = torch.full((nx * ny * 3,), 0.5, dtype=torch.float64, device=dev)
        tq = torch.full_like(ta, 0.5)
        tc = torch.full((nx * ny,), 5, dtype=torch.int32, device=dev)
        tl = torch.from_numpy(listed.astype(np.int32)).to(dev)
        st = ds.render_active(nx, ny, spp, DEPTH, seed, active=tl, accum=ta, accum_sq=tq, counts=tc, spp_begin=3,
                              spp_count=8)
        on = np.isin(np.arange(nx * ny), listed)
        want_a, want_q = np.where(np.repeat(on, 3), ref_a, 0.5), np.where(np.repeat(on, 3), ref_q, 0.5)
        assert np.array_equal(ta.cpu().numpy(), want_a) and np.array_equal(tq.cpu().numpy(), want_q)
        assert np.array_equal(tc.cpu().numpy(), np.where(on, 13, 5)) and st["samples"] == listed.size * 8
        # a bad device list is refused by the check kernel; nothing is written
        before = (ta.clone(), tq.clone(), tc.clone())
        for bad in ([7, 5, 9], [5, 5, 9], [5, 9, nx * ny], [0, 1, 2, 2], [3, 2]):
            tb = torch.tensor(bad, dtype=torch.int32, device=dev)
            with pytest.raises(_abi.RtwError, match="device pixel list") as e:
                ds.render_active(nx, ny, spp, DEPTH, seed, active=tb, accum=ta, accum_sq=tq, counts=tc, spp_begin=3,
                                 spp_count=8)
            assert "(-1)" in str(e.value)
        assert all(torch.equal(x, y) for x, y in zip((ta, tq, tc), before))
        # mixed kinds are refused in Python; through the C ABI a device list with host buffers is refused too
        with pytest.raises(ValueError):
            ds.render_active(nx, ny, spp, DEPTH, seed, active=listed, accum=ta)
        with pytest.raises(ValueError):
            ds.render_active(nx, ny, spp, DEPTH, seed, active=tl, accum=np.zeros(nx * ny * 3))
        host = np.full(nx * ny * 3, 0.5)
        prm = _abi.rtw_render_params(nx=nx, ny=ny, spp=spp, max_depth=DEPTH, seed=seed, row_step=1, spp_begin=3,
                                     spp_count=8, accum_on_device=0)
        rc = _abi.lib().rtw_render_accumulate_active(ds.handle, C.byref(sd.camera), C.byref(prm),
                                                     C.c_void_p(tl.data_ptr()), tl.numel(),
                                                     host.ctypes.data_as(C.c_void_p), None, None, None)
        assert rc == -1 and b"device pixel list with host buffers" in _abi.lib().rtw_last_error()
        assert (host == 0.5).all()
        # ... and a host buffer under accum_on_device
        prm.accum_on_device = 1
        rc = _abi.lib().rtw_render_accumulate_active(ds.handle, C.byref(sd.camera), C.byref(prm),
                                                     C.c_void_p(tl.data_ptr()), tl.numel(),
                                                     host.ctypes.data_as(C.c_void_p), None, None, None)
        assert rc == -1 and b"not device" in _abi.lib().rtw_last_error() and (host == 0.5).all()
    finally:
        ds.close()


@pytest.mark.parametrize("nx,ny", [(1, 1), (300, 7), (600, 500)])
def test_device_select_estimate_and_finalize(gpu, nx, ny):
    """One pixel; 2 100 pixels (9 blocks, the last partly filled); 300 000
    pixels (more than the 1 024 blocks the grids are capped at: several tiles
    per block)."""
    import torch
    s1, s2, counts = moments(nx, ny)
    rel, _, fin = rel_np(s1, s2, counts)
    judged = fin & (counts >= 2) & (counts < MAX_COUNT)
    half = float(np.median(rel[judged])) if judged.any() else 0.02
    ds = gpu.DeviceScene(gpu.SceneDesc("cornell_box", 1.0))
    try:
        t1, t2 = torch.from_numpy(s1).to("cuda:0"), torch.from_numpy(s2).to("cuda:0")
        tc = torch.from_numpy(counts.astype(np.int32)).to("cuda:0")
        for target in (1e9, 0.0, half):
            host = gpu.select_active(s1, s2, counts, nx, ny, target_rel=target, max_count=MAX_COUNT, floor=FLOOR)
            assert np.array_equal(host, active_np(s1, s2, counts, target, MAX_COUNT))
            got = ds.select_active(t1, t2, tc, nx, ny, target_rel=target, max_count=MAX_COUNT, floor=FLOOR)
            assert got.is_cuda and np.array_equal(got.cpu().numpy().astype(np.uint32), host), (nx, ny, target)
        se_h, sum_h = gpu.noise_estimate_counts(s1, s2, counts, nx, ny, FLOOR)
        se_d, sum_d = ds.noise_estimate_counts(t1, t2, tc, nx, ny, FLOOR)
        assert same_bits(se_d.cpu().numpy(), se_h), "the device map with counts differs from the host's"
        assert sum_d["pixels"] == sum_h["pixels"] and sum_d["nonfinite"] == sum_h["nonfinite"]
        for k in ("mean_rel", "max_rel", "rms_stderr"):
            assert sum_d[k] == pytest.approx(sum_h[k], rel=1e-9), k
        se_d2, sum_d2 = ds.noise_estimate_counts(t1, t2, tc, nx, ny, FLOOR)
        assert sum_d2 == sum_d and torch.equal(se_d2.view(torch.int64), se_d.view(torch.int64)), "not deterministic"
        # uniform counts: the uniform device estimator's bits, map and summary
        n = 7
        tu = torch.full((nx * ny,), n, dtype=torch.int32, device="cuda:0")
        se_u, sum_u = ds.noise_estimate(t1, t2, nx, ny, n, FLOOR)
        se_c, sum_c = ds.noise_estimate_counts(t1, t2, tu, nx, ny, FLOOR)
        assert torch.equal(se_u.view(torch.int64), se_c.view(torch.int64)) and sum_u == sum_c
        with np.errstate(all="ignore"):
            canvas = ds.finalize_counts(t1, tc, nx, ny).cpu().numpy()
            assert same_bits(canvas, gpu.finalize_counts(s1, counts, nx, ny))
            assert same_bits(ds.finalize_counts(t1, tu, nx, ny).cpu().numpy(), gpu.finalize(s1, nx, ny, n))
    finally:
        ds.close()


LOOP = dict(nx=60, ny=40, seed=7, min_spp=8, batch=8, max_spp=32)
_snapshots = {}


def loop_reference(gpu, scene, precision):
    """The whole image rendered in the loop's ranges through render_moments,
    with a snapshot after each; the target (the median rel_p of the 8-sample
    snapshot, from the definition in numpy) and what the loop must then do."""
    key = (scene, precision)
    if key in _snapshots:
        return _snapshots[key]
    nx, ny, seed = LOOP["nx"], LOOP["ny"], LOOP["seed"]
    ds = gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny))
    try:
        a, q = np.zeros(nx * ny * 3), np.zeros(nx * ny * 3)
        snaps = {}
        for begin in range(0, LOOP["max_spp"], LOOP["batch"]):
            ds.render_moments(nx, ny, LOOP["max_spp"], DEPTH, seed, spp_begin=begin, spp_count=LOOP["batch"], accum=a,
                              accum_sq=q, precision=precision)
            snaps[begin + LOOP["batch"]] = (a.copy(), q.copy())
    finally:
        ds.close()
    npix = nx * ny
    rel8, _, fin8 = rel_np(*snaps[8], np.full(npix, 8, np.uint32))
    assert fin8.all()
    target = float(np.median(rel8))
    counts = np.zeros(npix, dtype=np.uint32)
    live = np.ones(npix, dtype=bool)
    rounds = 0
    for n in sorted(snaps):
        if not live.any():
            break
        counts[live] = n
        rounds += 1
        still = np.zeros(npix, dtype=bool)
        still[active_np(*snaps[n], counts, target, LOOP["max_spp"]).astype(np.int64)] = True
        live &= still  # (a pixel that dropped out never comes back: its moments no longer change)
    share = float((counts > 8).mean())
    stops = {int(n): int((counts == n).sum()) for n in sorted(snaps)}
    print(f"{scene} {precision}: target {target:.5f}, active after round 0: {share:.3f}, pixels stopping at {stops}")
    _snapshots[key] = dict(snaps=snaps, target=target, counts=counts, rounds=rounds, share=share, stops=stops)
    return _snapshots[key]


@pytest.mark.parametrize("scene,precision,device_buffers", [("random_balls", "fp64", False), ("random_balls", "fp64", True),
                                                            ("cornell_box", "fp32", False)])
def test_the_loop(gpu, scene, precision, device_buffers):
    nx, ny, seed = LOOP["nx"], LOOP["ny"], LOOP["seed"]
    ref = loop_reference(gpu, scene, precision)
    # by construction about half the pixels go on after round 0 and some stop at
    # every count: otherwise the comparison below proves nothing
    assert 0.25 <= ref["share"] <= 0.75, ref["share"]
    assert all(v > 0 for v in ref["stops"].values()) and sorted(ref["stops"]) == [8, 16, 24, 32], ref["stops"]
    ds = gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny))
    try:
        r = gpu.render_adaptive(ds, nx, ny, LOOP["max_spp"], DEPTH, seed, target_rel=ref["target"],
                                min_spp=LOOP["min_spp"], batch=LOOP["batch"], floor=FLOOR, precision=precision,
                                device_buffers=device_buffers)
        _, summary = ds.noise_estimate_counts(r["accum"], r["accum_sq"], r["counts"], nx, ny, FLOOR, want_stderr=False)
        a, q, counts = r["accum"], r["accum_sq"], r["counts"]
        if device_buffers:
            assert a.is_cuda and q.is_cuda and counts.is_cuda
            a, q, counts = a.cpu().numpy(), q.cpu().numpy(), counts.cpu().numpy().astype(np.uint32)
    finally:
        ds.close()
    assert np.array_equal(counts, ref["counts"]), "the pixels' sample counts differ from the definition's"
    for n, (sa, sq) in ref["snaps"].items():
        at = np.repeat(counts == n, 3)
        assert np.array_equal(a[at], sa[at]) and np.array_equal(q[at], sq[at]), f"pixels that stopped at {n} samples"
    assert r["samples"] == int(counts.sum()) == r["stats"]["samples"]
    assert r["rounds"] == ref["rounds"] and r["pixels_at_max"] == int((counts == LOOP["max_spp"]).sum())
    assert r["summary"] == summary and summary["pixels"] == nx * ny
    assert [(b, c) for b, c, _ in r["history"]] == [(0, 8), (8, 8), (16, 8), (24, 8)][:r["rounds"]]
    assert [k for _, _, k in r["history"]] == [int((counts > b).sum()) for b, _, _ in r["history"]]
    assert r["samples"] < nx * ny * LOOP["max_spp"]


def test_cli(gpu, tmp_path):
    nx, ny, seed = LOOP["nx"], LOOP["ny"], LOOP["seed"]
    ref = loop_reference(gpu, "random_balls", "fp64")
    ds = gpu.DeviceScene(gpu.SceneDesc("random_balls", nx / ny))
    try:
        r = gpu.render_adaptive(ds, nx, ny, LOOP["max_spp"], DEPTH, seed, target_rel=ref["target"],
                                min_spp=LOOP["min_spp"], batch=LOOP["batch"], floor=FLOOR)
    finally:
        ds.close()
    out = tmp_path / "a.ppm"
    base = [str(CLI), "--scene", "random_balls", "--nx", str(nx), "--ny", str(ny), "--spp", str(LOOP["max_spp"]),
            "--depth", str(DEPTH), "--seed", str(seed), "--adaptive", repr(ref["target"]), "--min-spp",
            str(LOOP["min_spp"]), "--noise-batch", str(LOOP["batch"]), "--noise-floor", repr(FLOOR), "--out", str(out)]
    p = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"^Adaptive: rounds (\d+)  samples (\d+) of (\d+)  mean_rel (\S+)  max_rel (\S+)  at_max (\d+)$",
                  p.stdout, re.M)
    assert m, p.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(6))) == \
        (r["rounds"], r["samples"], nx * ny * LOOP["max_spp"], r["pixels_at_max"])
    assert float(m.group(4)) == pytest.approx(r["summary"]["mean_rel"], rel=1e-5)
    assert float(m.group(5)) == pytest.approx(r["summary"]["max_rel"], rel=1e-5)
    canvas = gpu.finalize_counts(r["accum"], r["counts"], nx, ny)
    want = (np.float64(np.float32(255.99)) * canvas).astype(np.int64).reshape(ny, nx, 3)[::-1].reshape(-1)
    tok = out.read_text().split()
    assert tok[:4] == ["P3", str(nx), str(ny), "255"]
    got = np.array(tok[4:], dtype=np.int64)
    assert got.size == want.size and (got != want).sum() <= max(1, want.size // 10000)
    p = subprocess.run(base + ["--gpus", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "one GPU" in p.stderr, p.stdout + p.stderr
