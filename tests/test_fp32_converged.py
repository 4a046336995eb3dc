"""tests/fp32_converged.py on synthetic renders: gamma-distributed samples
(skewed, as path radiance is) with a known mean per channel, so that the null
case, each planted error and the power condition have known answers.  No GPU."""
import copy

import numpy as np
import pytest

import fp32_converged as fc

NX, NY, N = 32, 24, 8192
SHAPE = 8.0          # gamma shape: coefficient of variation 1/sqrt(8) = 0.35
RATE = 5.3           # traversals per sample
# With cv = 0.35 and n = 8192 a channel's se / m is 0.39 % (cap 0.5 %) and the
# frame term 4 cv / sqrt(npix n) = 5.6e-4 of the level (cap 1e-3): enough
# power, and not much more, which is where the GPU tests run too.


def synthetic(seed, n=N, nx=NX, ny=NY, zero_channel=None):
    """A Render of n gamma samples per channel; channel means vary over the
    frame between 0.2 and 1.5 (the same for every seed)."""
    rng = np.random.default_rng(seed)
    npix = nx * ny
    mean = (0.2 + 1.3 * np.random.default_rng(0).random(npix * 3))
    S1 = np.zeros(npix * 3)
    S2 = np.zeros(npix * 3)
    step = 1024
    for _ in range(0, n, step):
        x = rng.gamma(SHAPE, 1.0 / SHAPE, size=(step, npix * 3)).astype(np.float64) * mean
        S1 += x.sum(axis=0)
        S2 += (x * x).sum(axis=0)
    if zero_channel is not None:
        k, value = zero_channel
        S1[k], S2[k] = n * value, n * value * value
    per_chunk = npix * n // fc.CHUNKS
    segments = [int(rng.poisson(RATE * per_chunk * 0.5) * 2) for _ in range(fc.CHUNKS)]  # over-dispersed counts
    return fc.Render(S1=S1, S2=S2, n=n, segments=segments, samples=[per_chunk] * fc.CHUNKS)


@pytest.fixture(scope="module")
def pair():
    return synthetic(1), synthetic(2)


def scaled(r, factor, pixels):
    """r with the samples of `pixels` (indices into ny*nx) multiplied by factor."""
    out = copy.deepcopy(r)
    S1, S2 = out.S1.reshape(-1, 3), out.S2.reshape(-1, 3)
    S1[pixels] *= factor
    S2[pixels] *= factor * factor
    return out


def test_moments():
    x = np.array([1.0, 2.0, 4.0, 9.0])
    r = fc.Render(S1=np.array([x.sum()] * 3), S2=np.array([(x * x).sum()] * 3), n=4, segments=[], samples=[])
    m, se2 = fc.mean_and_se2(r)
    assert np.allclose(m, 4.0) and np.allclose(se2, x.var(ddof=1) / 4)


def test_null_case_passes(pair):
    a, r = pair
    fc.power(r, NX, NY)
    for allowance in (fc.ALLOWANCE, 0.0):  # the control runs without the floor
        res = fc.compare(a, r, NX, NY, allowance)
        assert res.failures == [], res.row()
        assert 0.9 < res.z_rms < 1.1 and res.max_pixel_z < 5 and abs(res.frame_z) < 4
    assert fc.assert_same(a, r, NX, NY).failures == []


def test_frame_bias_fails_at_frame_scale_only(pair):
    a, r = pair
    res = fc.compare(scaled(a, 1.003, slice(None)), r, NX, NY)
    assert "frame" in res.failures and "block" not in res.failures and "pixel" not in res.failures, res.row()
    assert abs(res.rel_frame_diff - 0.003) < 1e-3
    with pytest.raises(AssertionError, match="frame"):
        fc.assert_same(scaled(a, 1.003, slice(None)), r, NX, NY)


def test_block_bias_fails_at_block_scale(pair):
    a, r = pair
    idx = np.arange(NX * NY).reshape(NY, NX)[8:12, 20:24].ravel()  # one 4x4 block of the tiling
    res = fc.compare(scaled(a, 1.05, idx), r, NX, NY)
    assert "block" in res.failures and "frame" not in res.failures, res.row()


def test_pixel_bias_fails_at_pixel_scale(pair):
    a, r = pair
    res = fc.compare(scaled(a, 1.30, np.array([5 * NX + 7])), r, NX, NY)
    assert "pixel" in res.failures and "frame" not in res.failures, res.row()
    assert res.max_pixel_z > 6


def test_traversal_shift_fails(pair):
    a, r = pair
    b = copy.deepcopy(a)
    b.segments = [int(round(s * 1.005)) for s in b.segments]
    res = fc.compare(b, r, NX, NY)
    assert res.failures == ["traversals"], res.row()
    assert res.traversals[0] / res.traversals[1] == pytest.approx(1.005, abs=1e-3)


def test_too_few_samples_is_no_power_not_a_verdict():
    a, r = synthetic(3, n=1024), synthetic(4, n=1024)
    with pytest.raises(fc.NoPower, match="no power"):
        fc.power(r, NX, NY)
    with pytest.raises(fc.NoPower):  # neither a pass nor an AssertionError
        fc.assert_same(a, r, NX, NY)
    # a planted error does not turn it into a failure either
    with pytest.raises(fc.NoPower):
        fc.assert_same(scaled(a, 1.30, slice(None)), r, NX, NY)


def test_zero_variance_channel_must_agree_within_the_floor():
    k = 3 * (7 * NX + 9) + 1
    r = synthetic(2, zero_channel=(k, 0.800))
    res = fc.compare(synthetic(1, zero_channel=(k, 0.808)), r, NX, NY)  # 1 % apart, floor 1e-3 * 0.85
    assert res.failures == ["zero_variance"], res.row()
    inside = fc.compare(synthetic(1, zero_channel=(k, 0.8004)), r, NX, NY)
    assert inside.failures == [], inside.row()
    # without the floor (the control) any difference fails
    assert fc.compare(synthetic(1, zero_channel=(k, 0.8004)), r, NX, NY, 0.0).failures == ["zero_variance"]


def test_rounding_jitter_is_not_sampling_variance(pair):
    """A channel that is one value in exact arithmetic, as the fp32 mode
    returns it: samples v (1 +- 2e-8) around a mean 5e-8 off.  Its computed se
    (2e-10 v) is rounding, and the 200 "standard errors" between the means
    must not reach the z-scores; the three scale rules still hold it to the
    floor."""
    a, r = copy.deepcopy(pair[0]), copy.deepcopy(pair[1])
    k, v = 3 * (11 * NX + 3) + 2, 0.5
    r.S1[k], r.S2[k] = N * v, N * v * v
    va = v * (1 + 5e-8)
    a.S1[k], a.S2[k] = N * va, N * va * va * (1 + 4e-16)
    m, se2 = fc.mean_and_se2(a)
    assert 0 < np.sqrt(se2[k]) < fc.RESOLUTION * m[k]
    res = fc.compare(a, r, NX, NY)
    assert res.failures == [] and res.max_pixel_z < 5 and res.z_rms < 1.1, res.row()
    # the same channel one per cent off is caught, jitter or not
    a.S1[k], a.S2[k] = N * v * 1.01, N * (v * 1.01) ** 2 * (1 + 4e-16)
    assert fc.compare(a, r, NX, NY).failures == ["zero_variance"]
    # a channel with sampling noise just above the resolution keeps its z
    b = copy.deepcopy(pair[0])
    b.S1[k], b.S2[k] = N * va, N * va * va * (1 + 4e-11)  # se = 7e-8 v
    assert fc.compare(b, r, NX, NY, 0.0).failures == []  # 5e-8 v apart: 0.7 se
    vb = v * (1 + 1e-6)                                   # 14 se apart
    b.S1[k], b.S2[k] = N * vb, N * vb * vb * (1 + 4e-11)
    assert "pixel" in fc.compare(b, r, NX, NY, 0.0).failures


def test_arguments():
    a, r = synthetic(1, n=1024, nx=8, ny=8), synthetic(2, n=1024, nx=8, ny=8)
    with pytest.raises(ValueError):
        fc.compare(a, r, 6, 8)  # no 4x4 tiling
    short = copy.deepcopy(a)
    short.segments = short.segments[:3]
    with pytest.raises(ValueError):
        fc.compare(short, r, 8, 8)
    bad = copy.deepcopy(a)
    bad.S1[0] = np.nan
    with pytest.raises(ValueError):
        fc.compare(bad, r, 8, 8)
