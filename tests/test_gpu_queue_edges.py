"""The persistent kernels' sample-queue reservation (csrc/rtw_queue.h's
arithmetic; rtw_kernels.hip reserve_samples in the fp32 kernels, the same
steps spelt out in the fp64 ones) at the sample counts where it can go
wrong: fewer samples than a wave wants, one short of and one past a wave, one
sample into the queue's second chunk, and every shard used with a partial last
chunk.  Depth 8; cornell_box flat takes the regrouping kernels (k_persist_sort,
k_fast_sort), random_balls with BVHs k_persist with LDS stacks and k_fast.

Every render hands out each sample once (stats["samples"]) and leaves a finite
accumulator.  In fp64 the persistent render equals the wavefront form's
(RTW_MODE=wavefront, a 1 000-path pool), whose k_regen reserves its samples
per block on its own, bit for bit and in its traversal count.  In both
precisions the 8-spp render equals itself in eight passes of 1 025 samples:
two chunks, the second holding one sample."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEPTH, SEED = 8, 9
SIZES = [  # nx, ny, spp
    (1, 1, 1),     # 1: fewer samples than a wave wants
    (7, 9, 1),     # 63: just under one wave
    (13, 5, 1),    # 65: just over one wave
    (41, 25, 1),   # 1 025: one sample into the second chunk
    (41, 25, 8),   # 8 200: every shard used, last chunk partial
]
SCENES = [("cornell_box", False), ("random_balls", True)]
_renders = {}  # (scene, bvh, size, precision) -> (accumulator, stats, kernel): rendered once, never written


@pytest.fixture(scope="module")
def gpu(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    return render


def _scene(gpu, scene, bvh, size):
    nx, ny, _ = size
    return gpu.DeviceScene(gpu.SceneDesc(scene, nx / ny, use_bvh=bvh))


def _default(gpu, scene, bvh, size, precision):
    key = (scene, bvh, size, precision)
    if key not in _renders:
        nx, ny, spp = size
        ds = _scene(gpu, scene, bvh, size)
        try:
            acc, st = ds.render_accumulate(nx, ny, spp, DEPTH, seed=SEED, precision=precision)
            q = ds.query()
        finally:
            ds.close()
        acc.setflags(write=False)
        _renders[key] = (acc, st, q["kernel_fast" if precision == "fp32" else "kernel"])
    return _renders[key]


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("scene,bvh", SCENES)
def test_every_sample_is_taken(gpu, scene, bvh, size, precision):
    acc, st, kernel = _default(gpu, scene, bvh, size, precision)
    nx, ny, spp = size
    print(f"QUEUE {scene} bvh={bvh} {nx}x{ny}x{spp} {precision}: {kernel}, samples {st['samples']}, "
          f"segments {st['segments']}")
    want = ("k_fast_sort<" if precision == "fp32" else "k_persist_sort<") if not bvh else \
           ("k_fast<" if precision == "fp32" else "k_persist<")
    assert kernel.startswith(want), kernel
    if bvh:  # the last template argument is LST: traversal stacks and the node packet in LDS
        assert kernel.endswith(", true>"), kernel
    assert st["samples"] == nx * ny * spp
    assert nx * ny * spp <= st["segments"] <= nx * ny * spp * DEPTH
    assert np.all(np.isfinite(acc))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("scene,bvh", SCENES)
def test_persistent_equals_wavefront(gpu, monkeypatch, scene, bvh, size):
    acc, st, _ = _default(gpu, scene, bvh, size, "fp64")
    nx, ny, spp = size
    monkeypatch.setenv("RTW_MODE", "wavefront")
    ds = _scene(gpu, scene, bvh, size)
    try:
        ref, st_ref = ds.render_accumulate(nx, ny, spp, DEPTH, seed=SEED, wavefront_paths=1000)
        kernel = ds.query()["kernel"]
    finally:
        ds.close()
    assert kernel.startswith(("k_segment<", "k_intersect<")), kernel
    assert st_ref["samples"] == st["samples"] == nx * ny * spp
    assert st["segments"] == st_ref["segments"]
    assert np.array_equal(acc, ref)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("scene,bvh", SCENES)
def test_passes_of_two_chunks(gpu, monkeypatch, scene, bvh, precision):
    size = SIZES[-1]
    acc, st, _ = _default(gpu, scene, bvh, size, precision)
    nx, ny, spp = size
    assert st["iterations"] == 1  # (the default budget: one pass)
    monkeypatch.setenv("RTW_PASS_SAMPLES", str(nx * ny))
    ds = _scene(gpu, scene, bvh, size)
    try:
        b, st_b = ds.render_accumulate(nx, ny, spp, DEPTH, seed=SEED, precision=precision)
    finally:
        ds.close()
    assert st_b["iterations"] == spp and st_b["samples"] == nx * ny * spp
    assert st_b["segments"] == st["segments"]
    assert np.array_equal(acc, b)
