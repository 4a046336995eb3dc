"""Ray queries on the GPU (include/rtw_query.h): rtw_trace_closest against the
host classes ray by ray (tests/cpp/host_rays.cpp), its t_max edges, the
oracle's recorded path segments, rtw_camera_rays against the feature kernel bit
for bit, rtw_trace_occluded against the closest hits, launch sizes, host and
device buffers, the refusals that need a device, and rtw_render --rays."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_gpu_denoise import FEATURE_CASES, _compile

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "raytracingweekend_amd"
CLI = PKG / "rtw_render"
F_MEDIA, F_WBVH, F_GBVH = 1, 2, 4
LISTED = (0, F_MEDIA, F_WBVH, F_GBVH, F_MEDIA | F_GBVH, F_WBVH | F_GBVH)  # rtw_select.h kIntersectList
N_RAYS = 2000
TOL = 1e-13  # the project's parity figure, relative to max(|value|, 1)

# (scene, bvh, form or None: from the handle's feature bits)
QUERY_CASES = [(c[0], c[1], c[5]) for c in FEATURE_CASES] + [("ties", False, None), ("ties", True, None),
                                                            ("ties_axis", False, None), ("ties_axis", True, None)]
IDS = [f"{c[0]}-{'bvh' if c[1] else 'flat'}" for c in QUERY_CASES]


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


# ---- the rays -----------------------------------------------------------------------
def _unit(rs, n):
    v = rs.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def make_rays(sd, seed=1, n=N_RAYS):
    """n rays (n, 8) and n minstd states for the scene of `sd`, from a seeded
    generator: a quarter each of camera rays towards random points of the
    world, rays from random points inside the world bounds in random directions
    of random length, rays aimed at primitive centres, and rays that start on a
    surface (a point of a sphere or a rect: their own hit at t ~ 0 falls to the
    t > 0.001f rule).  Times are random inside the shutter; a quarter of the
    rays have a finite random t_max, the others +inf.  All values finite."""
    d = sd.desc
    rs = np.random.default_rng(seed)
    cam = np.array(d.camera.origin[:])
    ent = [d.entries[e] for e in range(d.n_entries)]
    b = np.array([e.bounds[:] for e in ent])
    small = b[np.all(b[:, 3:] - b[:, :3] < 600.0, axis=1)]
    b = small if len(small) else b
    lo, hi = b[:, :3].min(axis=0), b[:, 3:].max(axis=0)
    size = float(np.linalg.norm(hi - lo))
    q = n // 4
    # primitive centres and surface points, in world space for prims of entries without ops
    centres, surface = [], []
    for k in range(d.n_prims):
        p = d.prims[k]
        if p.entry < 0:
            continue
        e = ent[p.entry]
        if e.n_ops:
            centres.append(0.5 * (np.array(e.bounds[:3]) + np.array(e.bounds[3:])))
            continue
        pp = p.p[:]
        if p.type in (0, 1):
            c, r = np.array(pp[:3]), abs(pp[3])
            centres.append(c)
            if p.type == 0 and r < 600.0:
                surface.append(("s", c, r))
        else:
            axis = {2: (0, 1, 2), 3: (0, 2, 1), 4: (1, 2, 0)}[p.type]  # (a, b, k) coordinates
            c = np.zeros(3)
            c[axis[0]], c[axis[1]], c[axis[2]] = 0.5 * (pp[0] + pp[1]), 0.5 * (pp[2] + pp[3]), pp[4]
            centres.append(c)
            surface.append(("r", axis, pp))
    centres = np.array(centres)
    o = np.empty((n, 3))
    dirs = np.empty((n, 3))
    # 1. from the camera towards the world
    o[:q] = cam
    dirs[:q] = lo + rs.random((q, 3)) * (hi - lo) - cam
    # 2. inside the bounds, any direction, any length
    o[q:2 * q] = lo + rs.random((q, 3)) * (hi - lo)
    dirs[q:2 * q] = _unit(rs, q) * np.exp(rs.uniform(-3, 3, (q, 1)))
    # 3. aimed at primitive centres, from the camera or from inside
    o[2 * q:3 * q] = np.where(rs.random((q, 1)) < 0.5, cam, lo + rs.random((q, 3)) * (hi - lo))
    # (a thousandth of the world off the centre: a camera level with a rect's plane would otherwise get a direction
    # with a component of exactly 0 and the reference's own 0 / 0 for that rect's t)
    dirs[2 * q:3 * q] = centres[rs.integers(0, len(centres), q)] + 1e-3 * size * rs.standard_normal((q, 3)) - o[2 * q:3 * q]
    # 4. starting on a surface
    if not surface:  # (no plain sphere or rect: the centres, which lie inside)
        surface = [("s", c, 0.0) for c in centres]
    for k in range(3 * q, n):
        kind, a, r = surface[rs.integers(0, len(surface))]
        if kind == "s":
            o[k] = a + r * _unit(rs, 1)[0]
        else:
            pt = np.zeros(3)
            pt[a[0]], pt[a[1]], pt[a[2]] = rs.uniform(r[0], r[1]), rs.uniform(r[2], r[3]), r[4]
            o[k] = pt
    dirs[3 * q:] = _unit(rs, n - 3 * q)
    dirs[np.all(dirs == 0, axis=1)] = (0.0, 1.0, 0.0)
    t0, t1 = sorted((d.camera.time0, d.camera.time1))
    rays = np.empty((n, 8))
    rays[:, :3], rays[:, 3:6] = o, dirs
    rays[:, 6] = rs.uniform(t0, t1, n)
    rays[:, 7] = np.where(rs.random(n) < 0.25, rs.uniform(0.0, size, n) / np.linalg.norm(dirs, axis=1), np.inf)
    assert np.isfinite(rays[:, :7]).all() and np.all(dirs != 0)
    rng = rs.integers(1, 2147483646, n).astype(np.uint32)
    return rays, rng


# ---- the host classes, once per set of rays ----------------------------------------------
@pytest.fixture(scope="module")
def host_rays(built, tmp_path_factory):
    exe = _compile("host_rays.cpp", tmp_path_factory.mktemp("host_rays") / "host_rays")
    cache = {}

    def run(scene, key, rays, rng):
        """(hit flags, t, p, n, rng after) of tests/cpp/host_rays.cpp."""
        if (scene, key) not in cache:
            base = exe.parent / f"{scene}_{key}"
            rays.tofile(f"{base}.rays")
            rng.tofile(f"{base}.rng")
            r = subprocess.run([str(exe), scene, f"{base}.rays", f"{base}.rng", f"{base}.out"], capture_output=True,
                               text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            n = len(rays)
            raw = np.fromfile(f"{base}.out", dtype=np.uint8)
            rec = raw[:n * 64].view(np.float64).reshape(n, 8).copy()
            after = raw[n * 64:].view(np.uint32).copy()
            rec.setflags(write=False), after.setflags(write=False)
            cache[(scene, key)] = (rec[:, 0] == 1.0, rec[:, 1], rec[:, 2:5], rec[:, 5:8], after)
        return cache[(scene, key)]
    return run


def relerr(got, want):
    return np.abs(got - want) / np.maximum(np.abs(want), 1.0)


def compare(hits, host, what):
    """The hit flag exact; t, p, n of the hits within TOL; returns the hit mask."""
    hit, t, p, n, _ = host
    got = hits["prim"] != -1
    assert np.array_equal(got, hit), f"{what}: hit flags differ at {np.flatnonzero(got != hit)[:8]}"
    e = [relerr(hits["t"][hit], t[hit]).max(initial=0.0), relerr(hits["p"][hit], p[hit]).max(initial=0.0),
         relerr(hits["n"][hit], n[hit]).max(initial=0.0)]
    same = (np.array_equal(hits["t"][hit], t[hit]) and np.array_equal(hits["p"][hit], p[hit])
            and np.array_equal(hits["n"][hit], n[hit]))
    print(f"{what}: {int(hit.sum())} of {len(hit)} rays hit; max error t {e[0]:.3e} p {e[1]:.3e} n {e[2]:.3e}; "
          f"bit-identical: {same}")
    assert max(e) <= TOL, what
    return hit


def check_misses(rays, hits, miss):
    """prim = material = -1, t = t_max as given, p = n = 0."""
    assert np.all(hits["prim"][miss] == -1) and np.all(hits["material"][miss] == -1)
    assert np.array_equal(hits["t"][miss], rays[miss, 7], equal_nan=True)
    assert not hits["p"][miss].any() and not hits["n"][miss].any()


def form_of(ds):
    f = ds.query()["features"] & 7
    return f if f in LISTED else F_MEDIA | F_GBVH


# ---- 1. against the host classes, 5. occlusion ----------------------------------------------
@pytest.mark.parametrize("scene,bvh,form", QUERY_CASES, ids=IDS)
def test_closest_hits_match_the_host_classes(gpu, host_rays, scene, bvh, form):
    """All six traversal forms of k_query, and the coincident geometry of `ties`
    and `ties_axis`: the hit flag exact, t, p and n within 1e-13 relative to
    max(|value|, 1), the rng states after equal (media scenes draw, the others
    leave them alone), material = the prim's, or a medium's phase material; and
    rtw_trace_occluded = (prim != -1) with, for media, the closest call's
    states."""
    sd = gpu.SceneDesc(scene, 1.0, use_bvh=bvh)
    rays, rng0 = make_rays(sd)
    host = host_rays(scene, "base", rays, rng0)
    ds = gpu.DeviceScene(sd)
    try:
        names = ds.query_trace()
        f = form_of(ds)
        media = bool(f & F_MEDIA)
        rng = rng0.copy()
        hits = ds.trace_rays(rays, rng if media else None)
        st = ds.last_query_stats
        rng_o = rng0.copy()
        occ = ds.trace_rays(rays, rng_o if media else None, occluded=True)
    finally:
        ds.close()
    if form is not None:
        assert f == form
    assert names == (f"k_query<{f}>", f"k_occluded<{f}>"), names
    assert st["samples"] == N_RAYS and st["segments"] == N_RAYS and st["launches_intersect"] == 1 and st["ms_total"] > 0
    hit = compare(hits, host, f"{scene} {'bvh' if bvh else 'flat'} {names[0]}")
    assert hit.any() and (~hit).any(), "the rays should both hit and miss"
    check_misses(rays, hits, ~hit)
    assert np.array_equal(rng, host[4]), "rng states after the query"
    if not media:
        assert np.array_equal(rng, rng0)
    d = sd.desc
    prim, mat = hits["prim"], hits["material"]
    on_prim = prim >= 0
    assert np.all(prim[hit] != -1) and np.all(prim < d.n_prims)
    want = np.array([d.prims[int(k)].material for k in prim[on_prim]], dtype=np.int32)
    assert np.array_equal(mat[on_prim], want)
    medium = prim <= -2
    assert media or not medium.any()
    for k in np.flatnonzero(medium):
        e = d.entries[int(-prim[k] - 2)]
        assert e.kind == 1 and mat[k] == e.phase_material
    if scene in ("book2_final", "nested"):
        assert medium.any(), "no ray ended in a medium"
    # 5. occlusion
    assert occ.dtype == np.uint8 and np.array_equal(occ, (prim != -1).astype(np.uint8))
    assert np.array_equal(rng_o, rng)


# ---- 2. t_max edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,bvh", [("cornell_box", False), ("random_balls", False), ("random_balls", True)],
                         ids=["cornell_box-flat", "random_balls-flat", "random_balls-bvh"])
def test_t_max_edges(gpu, host_rays, scene, bvh):
    """Every hit of test 1 queried again with t_max = t, the double below and
    the double above: all three as the host classes answer (a rect at exactly
    t_max is accepted, a sphere is not).  t_max = 0.0005, NaN and -1 are
    misses with the record the header states."""
    sd = gpu.SceneDesc(scene, 1.0, use_bvh=bvh)
    rays, rng0 = make_rays(sd)
    hit, t, _, _, _ = host_rays(scene, "base", rays, rng0)
    base = rays[hit].copy()
    edges = np.concatenate([base, base, base])
    m = len(base)
    edges[:m, 7] = t[hit]
    edges[m:2 * m, 7] = np.nextafter(t[hit], 0.0)
    edges[2 * m:, 7] = np.nextafter(t[hit], np.inf)
    host = host_rays(scene, "edges", edges, np.ones(3 * m, dtype=np.uint32))
    bad = np.concatenate([base[:30], base[:30], base[:30]])
    bad[:30, 7], bad[30:60, 7], bad[60:, 7] = 0.0005, np.nan, -1.0
    ds = gpu.DeviceScene(sd)
    try:
        hits = ds.trace_rays(edges)
        none = ds.trace_rays(bad)
        occ = ds.trace_rays(bad, occluded=True)
    finally:
        ds.close()
    got = compare(hits, host, f"{scene} {'bvh' if bvh else 'flat'} t_max edges")
    check_misses(edges, hits, ~got)
    # the double above always keeps the hit; equality keeps exactly the rects among the same winners
    assert got[2 * m:].all()
    d = sd.desc
    first = hits["prim"][2 * m:]
    is_rect = np.array([d.prims[int(k)].type >= 2 for k in first])
    same_winner = hits["prim"][:m] == first
    print(f"  at t_max = t: {int(got[:m].sum())} of {m} still hit ({int(is_rect.sum())} rect winners)")
    assert np.all(same_winner[is_rect]) and not np.any(same_winner[~is_rect])
    if scene == "cornell_box":
        assert is_rect.any()
    else:
        assert (~is_rect).any()
    check_misses(bad, none, np.ones(len(bad), dtype=bool))
    assert not occ.any()


# ---- 3. the oracle's segments -------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cornell_box", "random_balls", "dielectric", "light_sample"])
def test_oracle_segments(gpu, scene):
    """Every segment (o, d, time) the oracle records along 192 paths of depth
    50, asked with t_max = inf: the hit flags exact, t within 1e-13 relative
    of the recorded one."""
    from oracle_lib import oracle
    nx, ny, depth, seed = 16, 12, 50, 5
    sd = gpu.SceneDesc(scene, nx / ny)
    L = oracle()
    rows = []
    buf = np.zeros((64, 8))
    rad = (C.c_double * 3)()
    for j in range(ny):
        for i in range(nx):
            k = L.rtw_oracle_trace(sd.ptr, C.byref(sd.camera), nx, ny, i, j, 0, depth, seed, rad,
                                   buf.ctypes.data_as(C.c_void_p), len(buf))
            assert 1 <= k <= len(buf)
            rows.append(buf[:k].copy())
    seg = np.concatenate(rows)
    rays = np.empty((len(seg), 8))
    rays[:, :6], rays[:, 6], rays[:, 7] = seg[:, :6], seg[:, 7], np.inf
    assert np.isfinite(rays[:, :7]).all()
    ds = gpu.DeviceScene(sd)
    try:
        hits = ds.trace_rays(rays)
    finally:
        ds.close()
    hit = seg[:, 6] != -1.0
    assert np.array_equal(hits["prim"] != -1, hit)
    err = relerr(hits["t"][hit], seg[hit, 6]).max()
    print(f"{scene}: {len(seg)} segments of {nx * ny} paths, {int(hit.sum())} hits, max t error {err:.3e}, "
          f"bit-identical: {np.array_equal(hits['t'][hit], seg[hit, 6])}")
    assert len(seg) > nx * ny and hit.any() and (~hit).any()
    assert err <= TOL


# ---- 4. camera rays reproduce the feature kernel --------------------------------------------------------
@pytest.mark.parametrize("scene,bvh,nx,ny,spp,form", FEATURE_CASES,
                         ids=[f"{c[0]}-{'bvh' if c[1] else 'flat'}" for c in FEATURE_CASES])
def test_camera_rays_reproduce_the_feature_kernel(gpu, scene, bvh, nx, ny, spp, form):
    """camera_rays of one sample, traced with the returned states, against
    render_features of that sample into zeros: coverage, 1 / t and the normal
    as exact bits; a row shard holds the same rays at its own q."""
    seed = 7
    ds = gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny, use_bvh=bvh))
    try:
        for s in (0, 3 if spp > 3 else spp - 1):
            rays, rng = ds.camera_rays(nx, ny, spp, seed, spp_begin=s, spp_count=1)
            assert rays.shape == (nx * ny, 8) and np.all(np.isposinf(rays[:, 7]))
            hits = ds.trace_rays(rays, rng.copy())
            feat, _ = ds.render_features(nx, ny, spp, seed, spp_begin=s, spp_count=1)
            feat = feat.reshape(-1, 8)
            hit = hits["prim"] != -1
            assert np.array_equal(feat[:, 7], hit.astype(np.float64))
            with np.errstate(divide="ignore"):
                assert np.array_equal(feat[:, 6], np.where(hit, 1.0 / hits["t"], 0.0))
            assert np.array_equal(feat[:, 3:6], hits["n"])
            assert hit.any()
            # rows 1, 4, 7, ...: the same rays and states, at q = row * nx + i of the shard
            shard, shard_rng = ds.camera_rays(nx, ny, spp, seed, spp_begin=s, spp_count=1, row_begin=1, row_step=3)
            whole = rays.reshape(ny, nx, 8)[1::3].reshape(-1, 8)
            assert np.array_equal(shard, whole) and np.array_equal(shard_rng, rng.reshape(ny, nx)[1::3].ravel())
        # two samples in one call: sample-major q; device tensors hold the same bytes
        two, two_rng = ds.camera_rays(nx, ny, spp, seed, spp_begin=0, spp_count=2)
        one, one_rng = ds.camera_rays(nx, ny, spp, seed, spp_begin=1, spp_count=1)
        assert np.array_equal(two[nx * ny:], one) and np.array_equal(two_rng[nx * ny:], one_rng)
        dev, dev_rng = ds.camera_rays(nx, ny, spp, seed, spp_begin=0, spp_count=2, device=True)
        assert np.array_equal(dev.cpu().numpy(), two) and np.array_equal(dev_rng.cpu().numpy().view(np.uint32), two_rng)
    finally:
        ds.close()


# ---- 6. sizes and buffers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,bvh", [("cornell_box", False), ("nested", False)], ids=["cornell_box", "nested"])
def test_sizes_and_buffers(gpu, scene, bvh):
    """n = 1, 63, 64, 65, a block + 1 and more than a full grid pass (the launch
    uses min(ceil(n / 256), 8 blocks per CU) blocks of 256 threads: query_trace
    in rtw_kernels.hip), which for host buffers is also more than one staged
    chunk: every ray's record is the one the 2 000-ray call of test 1 gave,
    from host buffers and from torch tensors, byte for byte."""
    import torch
    sd = gpu.SceneDesc(scene, 1.0, use_bvh=bvh)
    rays, rng0 = make_rays(sd)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    full = cus * 8 * 256
    ds = gpu.DeviceScene(sd)
    try:
        media = bool(form_of(ds) & F_MEDIA)
        rng = rng0.copy()
        base = ds.trace_rays(rays, rng if media else None)
        for n in (1, 63, 64, 65, 257, full + 77):
            idx = np.arange(n) % N_RAYS
            r_n, g_n = np.ascontiguousarray(rays[idx]), rng0[idx].copy()
            h_host = ds.trace_rays(r_n, g_n if media else None)
            assert np.array_equal(h_host.view(np.uint8), base[idx].view(np.uint8)), n
            o_host = ds.trace_rays(r_n, rng0[idx].copy() if media else None, occluded=True)
            assert np.array_equal(o_host, (base["prim"][idx] != -1).astype(np.uint8)), n
            r_dev = torch.from_numpy(r_n).cuda()
            g_dev = torch.from_numpy(rng0[idx].astype(np.int32)).cuda() if media else None
            h_dev = ds.trace_rays(r_dev, g_dev)
            torch.cuda.synchronize()
            assert np.array_equal(h_dev["records"].cpu().numpy().view(np.uint8).ravel(), h_host.view(np.uint8).ravel()), n
            assert np.array_equal(h_dev["prim"].cpu().numpy(), h_host["prim"])
            assert np.array_equal(h_dev["material"].cpu().numpy(), h_host["material"])
            assert np.array_equal(h_dev["t"].cpu().numpy(), h_host["t"])
            if media:
                assert np.array_equal(g_dev.cpu().numpy().view(np.uint32), g_n) and np.array_equal(g_n, rng[idx])
            g_dev = torch.from_numpy(rng0[idx].astype(np.int32)).cuda() if media else None
            o_dev = ds.trace_rays(r_dev, g_dev, occluded=True)
            assert np.array_equal(o_dev.cpu().numpy(), o_host), n
        stats = ds.last_query_stats
        assert stats["samples"] == full + 77 and stats["launches_intersect"] == 1
        # n == 0 is a successful no-op
        assert len(ds.trace_rays(np.empty((0, 8)))) == 0
    finally:
        ds.close()


def test_refusals_that_need_a_device(gpu):
    """A misaligned device pointer, host memory passed with on_device, a media
    scene without rng, an output over its input, fp32, a ray outside the
    shutter of a BVH scene with moving spheres (host and device buffers
    alike), and the strict build."""
    import torch
    from raytracingweekend_amd import _abi
    from raytracingweekend_amd._abi import RtwError
    L = _abi.lib()
    sd = gpu.SceneDesc("random_balls", 1.0, use_bvh=True)
    rays, _ = make_rays(sd, n=64)
    ds = gpu.DeviceScene(sd)
    try:
        dev = torch.from_numpy(rays).cuda()
        out = torch.empty((65, 8), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        prm = _abi.rtw_query_params(on_device=1)
        call = lambda r, o, p=prm, n=64: L.rtw_trace_closest(ds.handle, C.c_void_p(r), n, None, C.byref(p),
                                                             C.c_void_p(o), None)
        assert call(dev.data_ptr(), out.data_ptr()) == 0
        assert call(dev.data_ptr(), out.data_ptr() + 8) == -1 and b"aligned" in L.rtw_last_error()
        assert call(dev.data_ptr() + 8, out.data_ptr(), n=63) == -1
        assert call(rays.ctypes.data, out.data_ptr()) == -1          # host memory passed as device memory
        assert call(dev.data_ptr(), dev.data_ptr()) == -1 and b"overlap" in L.rtw_last_error()
        assert call(dev.data_ptr(), out.data_ptr(), _abi.rtw_query_params(on_device=1, precision=1)) == -5
        assert call(dev.data_ptr(), out.data_ptr(), n=0) == 0
        # the shutter: random_balls' spheres move, the BVH's boxes cover the desc camera's shutter only
        t0, t1 = sorted((sd.camera.time0, sd.camera.time1))
        assert t1 > t0
        late = rays.copy()
        late[17, 6] = t1 + 0.5
        for r in (late, torch.from_numpy(late).cuda()):
            with pytest.raises(RtwError, match="shutter"):
                ds.trace_rays(r)
            with pytest.raises(RtwError, match="shutter"):
                ds.trace_rays(r, occluded=True)
        assert len(ds.trace_rays(rays)) == 64  # the handle still serves
        with pytest.raises(RtwError):
            ds.camera_rays(8, 8, 1, 0, spp_count=5)  # more samples than spp
    finally:
        ds.close()
    # flat, the same scene traces any time
    ds = gpu.DeviceScene(gpu.SceneDesc("random_balls", 1.0))
    try:
        assert len(ds.trace_rays(late)) == 64
    finally:
        ds.close()
    ds = gpu.DeviceScene(gpu.SceneDesc("nested", 1.0))
    try:
        with pytest.raises(RtwError, match="media"):
            ds.trace_rays(rays)
        with pytest.raises(RtwError, match="media"):
            ds.trace_rays(rays, occluded=True)
    finally:
        ds.close()
    # the strict build has the symbols and refuses
    strict = _abi.load_library(PKG / "_build" / "librtw_strict.so")
    a, b = C.create_string_buffer(128), C.create_string_buffer(128)
    fake = C.c_int(0)
    assert strict.rtw_scene_query_trace(C.byref(fake), a, b) == -5
    prm = _abi.rtw_query_params()
    hits = np.zeros((64, 8))
    assert strict.rtw_trace_closest(C.byref(fake), rays.ctypes.data_as(C.c_void_p), 64, None, C.byref(prm),
                                    hits.ctypes.data_as(C.c_void_p), None) == -5


# ---- 7. the CLI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,bvh", [("random_balls", True), ("nested", False)], ids=["random_balls-bvh", "nested"])
def test_cli_round_trip(gpu, tmp_path, scene, bvh):
    """rtw_render --rays / --hits (and --occluded, --rng) gives trace_rays'
    bytes and one Query: line naming the kernel."""
    sd = gpu.SceneDesc(scene, 1.0, use_bvh=bvh)
    rays, rng0 = make_rays(sd, n=500)
    ds = gpu.DeviceScene(sd)
    try:
        media = bool(form_of(ds) & F_MEDIA)
        rng = rng0.copy()
        want = ds.trace_rays(rays, rng if media else None)
        names = ds.query_trace()
    finally:
        ds.close()
    rays.tofile(tmp_path / "rays.bin")
    for k, occluded in enumerate((False, True)):
        rng0.tofile(tmp_path / "rng.bin")
        out = tmp_path / f"hits{k}.bin"
        cmd = [str(CLI), "--scene", scene, "--nx", "100", "--ny", "100", *(["--bvh"] if bvh else []), "--rays",
               str(tmp_path / "rays.bin"), "--hits", str(out), *(["--occluded"] if occluded else []),
               *(["--rng", str(tmp_path / "rng.bin")] if media else [])]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        lines = [l for l in p.stdout.splitlines() if l.startswith("Query:")]
        assert len(lines) == 1, p.stdout
        m = re.fullmatch(r"Query: (k_\w+<\d+>)  rays 500  [0-9.]+ ms", lines[0])
        assert m and m.group(1) == names[int(occluded)], lines[0]
        if occluded:
            assert np.array_equal(np.fromfile(out, dtype=np.uint8), (want["prim"] != -1).astype(np.uint8))
        else:
            assert out.read_bytes() == want.tobytes()
        if media:
            assert np.array_equal(np.fromfile(tmp_path / "rng.bin", dtype=np.uint32), rng)
    if media:
        p = subprocess.run(cmd[:-2], capture_output=True, text=True, timeout=120)
        assert p.returncode == 1 and "media" in p.stderr
