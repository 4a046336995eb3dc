"""The fp32 fast mode (rtw_render_params.precision = RTW_PRECISION_FP32,
rtw_fast.h) against the oracle: statistical parity.

The reference computes in double (vec3.h:35-44) and the fp64 mode matches it
sample for sample (tests/test_gpu_parity.py).  The fast mode draws and rounds
differently (one raw minstd_rand draw per uniform, single precision), so its
image is another Monte-Carlo estimate of the same expectation; the test asks
that it be indistinguishable from one:

* per 8x8-pixel block b, d_b = fast mean - oracle mean (linear radiance) and
  e_b = fp64-mode mean with another seed - oracle mean.  fp64 with another
  seed is the reference's estimator with independent noise, so without bias
  d_b and e_b share one distribution.  Three fast-mode seeds and three other
  fp64 seeds are averaged (the scenes' light paths are heavy-tailed: a few
  fireflies dominate one render's block variance):
    - spread:  mean(d_b^2) < 2 mean(e_b^2)  (F-ratio over >= 96 block
      differences, 32+ blocks x 3 renders; the 99.9th percentile of
      F(96, 96) is about 1.9)
    - bias:    |mean(d_b)| < 4 sqrt(mean(e_b^2) / 3B) + 1e-3 |image mean|
* traversals per sample within 3 % of the fp64 mode's (same paths in law).

The statistic itself lives in tests/fp32_stats.py (test_gpu_bvh_forms.py
applies it to Normal-mode renders).
"""
import numpy as np
import pytest

import fp32_stats
from oracle_lib import oracle_sums

pytestmark = pytest.mark.gpu

# scene, nx, ny, spp, depth, bvh
CASES = [
    ("cornell_box", 64, 64, 64, 50, False),
    ("random_balls", 96, 64, 16, 50, False),
    ("random_balls", 96, 64, 16, 50, True),
    ("dielectric", 64, 32, 64, 50, False),
    ("light_sample", 64, 32, 64, 50, False),
    ("book2_final", 64, 64, 16, 50, False),
    ("book2_final", 64, 64, 16, 50, True),
    ("nested", 48, 48, 32, 50, False),
    # group BVHs without media: k_fast<F_GBVH> and k_fast<F_WBVH | F_GBVH>
    ("grouped", 96, 64, 16, 50, True),
    ("grouped_world", 96, 64, 16, 50, True),
    # coincident primitives (hits at equal distance), list walks and BVHs
    ("ties", 96, 64, 16, 50, False),
    ("ties", 96, 64, 16, 50, True),
]


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


@pytest.mark.parametrize("scene,nx,ny,spp,depth,bvh", CASES,
                         ids=[f"{c[0]}{'_bvh' if c[5] else ''}" for c in CASES])
def test_fast_mode_is_statistically_the_reference(gpu, scene, nx, ny, spp, depth, bvh):
    sd = gpu.SceneDesc(scene, nx / ny, use_bvh=bvh)
    ds = gpu.DeviceScene(sd)
    try:
        fast, other = fp32_stats.render_sets(ds, nx, ny, spp, depth)
        info = ds.query()
    finally:
        ds.close()
    ref, seg_ref = oracle_sums(gpu.SceneDesc(scene, nx / ny), nx, ny, spp, depth, fp32_stats.REF_SEED)
    for acc, st in fast:
        assert st["samples"] == nx * ny * spp and np.all(np.isfinite(acc))
        assert st["bytes_intersect"] == 36 * st["segments"]
    assert info["kernel_fast"].startswith(("k_fast<", "k_fast_sort<"))
    fp32_stats.assert_statistically_the_reference([a for a, _ in fast], [a for a, _ in other], ref, nx, ny, spp)
    seg32 = sum(st["segments"] for _, st in fast)
    seg64 = sum(st["segments"] for _, st in other)
    assert abs(seg32 / seg64 - 1) < 0.03
    assert abs(seg64 / 3 / seg_ref - 1) < 0.03


def test_fast_mode_shards_and_passes(gpu, monkeypatch):
    """The fast mode keeps the render loop's contract: sample shards add up
    to the whole range (each sample owns its stream, so exactly, up to fp64
    reassociation of the shard sums), and a render split into passes equals
    the one-pass render bit for bit."""
    nx, ny, spp, depth = 80, 60, 8, 50
    sd = gpu.SceneDesc("cornell_box", nx / ny)
    ds = gpu.DeviceScene(sd)
    try:
        whole, st = ds.render_accumulate(nx, ny, spp, depth, seed=3, precision="fp32")
        parts = np.zeros_like(whole)
        ds.render_accumulate(nx, ny, spp, depth, seed=3, spp_begin=0, spp_count=5, accum=parts, precision="fp32")
        ds.render_accumulate(nx, ny, spp, depth, seed=3, spp_begin=5, spp_count=3, accum=parts, precision="fp32")
        monkeypatch.setenv("RTW_PASS_SAMPLES", str(nx * ny * 3))
        passes, st3 = ds.render_accumulate(nx, ny, spp, depth, seed=3, precision="fp32")
    finally:
        ds.close()
    assert np.allclose(parts, whole, rtol=1e-12, atol=1e-12)
    assert st3["launches_intersect"] == 3 and np.array_equal(passes, whole)
    assert st3["segments"] == st["segments"]


def _render_child(env, scene, nx, ny, spp, depth, seed, bvh, precision):
    """Render in a fresh process with extra environment (RTW_LDS_NODES is
    read per launch, but a child keeps the switch away from this process)."""
    import os
    import subprocess
    import sys
    import tempfile
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    with tempfile.TemporaryDirectory() as td:
        out = Path(td) / "acc.npy"
        code = (f"import sys; sys.path.insert(0, {str(root)!r}); import numpy as np; "
                f"from raytracingweekend_amd import render as r; "
                f"ds = r.DeviceScene(r.SceneDesc({scene!r}, {nx}/{ny}, use_bvh={bvh})); "
                f"a, st = ds.render_accumulate({nx}, {ny}, {spp}, {depth}, seed={seed}, precision={precision!r}); "
                f"ds.close(); np.save({str(out)!r}, a); print('SEGMENTS', st['segments'])")
        r = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, check=True, timeout=300,
                           capture_output=True, text=True)
        segs = int(r.stdout.split("SEGMENTS")[-1].split()[0])
        return np.load(out), segs


@pytest.mark.parametrize("scene", ["random_balls", "book2_final"])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_node_packet_changes_no_sample(gpu, scene, precision):
    """The BVH node packet (the top nodes staged in LDS: k_persist for fp64,
    k_fast for fp32) only changes where a node is read from: the render with
    it equals the render without it (RTW_LDS_NODES=0) bit for bit, with the
    same traversal count."""
    nx, ny, spp, depth = 96, 64, 4, 50
    with_p, s1 = _render_child({}, scene, nx, ny, spp, depth, 7, True, precision)
    without, s0 = _render_child({"RTW_LDS_NODES": "0"}, scene, nx, ny, spp, depth, 7, True, precision)
    assert s1 == s0 and np.array_equal(with_p, without)
    assert np.all(np.isfinite(with_p)) and with_p.sum() > 0


@pytest.mark.parametrize("bvh", [True, False])
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
def test_box_table_changes_no_sample(gpu, bvh, precision):
    """Box items read their six rects from one planes record (scene::boxes,
    rtw_scene_upload, when every box's rects match the box's planes): the
    Book-2 render with the table equals the render that reads the rects
    (RTW_BOX_TABLE=0) bit for bit, with the same traversal count -- in the
    group-BVH walks (bvh) and with the flat list, which has no box items."""
    nx, ny, spp, depth = 96, 64, 4, 50
    with_t, s1 = _render_child({}, "book2_final", nx, ny, spp, depth, 11, bvh, precision)
    without, s0 = _render_child({"RTW_BOX_TABLE": "0"}, "book2_final", nx, ny, spp, depth, 11, bvh, precision)
    assert s1 == s0 and np.array_equal(with_t, without)
    assert np.all(np.isfinite(with_t)) and with_t.sum() > 0


def test_cli_precision_switch(tmp_path):
    """The reference-main equivalent (rtw_render) renders in either precision
    (--precision fp64|fp32, SURVEY.md §5's config row) and writes its PPM."""
    import subprocess
    from raytracingweekend_amd import build
    cli = build.CLI
    assert cli.exists(), "rtw_render is built by raytracingweekend_amd.build (build())"
    for prec in ("fp64", "fp32"):
        out = tmp_path / f"{prec}.ppm"
        r = subprocess.run([str(cli), "--scene", "cornell_box", "--nx", "32", "--ny", "32", "--spp", "4",
                            "--depth", "20", "--precision", prec, "--out", str(out)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        assert "Msamples/s" in r.stdout
        assert out.read_text().startswith("P3\n32 32\n255\n")
