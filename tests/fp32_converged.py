"""The statistic that compares two converged renders of one scene from their
per-pixel moments (tests/test_gpu_fp32_probes.py applies it to the fp32 fast
mode against the fp64 mode; tests/test_fp32_converged.py tests it on synthetic
samples).  Pure numpy, no tests here.

A render is a `Render`: the per-channel sums S1 and sums of squares S2 of n
samples per pixel (DeviceScene.render_moments), taken in CHUNKS equal sample
ranges whose traversal counts are kept.  Per channel

    m = S1 / n,    se^2 = max(S2 - S1 m, 0) / ((n - 1) n)

and with `level` the reference's mean m over the frame and floor = allowance *
level (allowance 1e-3: what tests/fp32_stats.py already grants the fast mode),
A (under test) is compared with R (reference) at three scales, every pixel in
every one, per colour channel:

    pixel      |mA - mR|      <= 6 sqrt(seA^2 + seR^2)      + floor
    4x4 block  |sum(mA - mR)| <= 5 sqrt(sum(seA^2 + seR^2)) + 16 floor
    frame      |sum(mA - mR)| <= 4 sqrt(sum(seA^2 + seR^2)) + npix floor

(a channel without variance in either render must agree within the floor: the
pixel rule with se = 0, reported as its own failure); the rms of the pixel
z-scores over channels with se > 0 must stay below 1.1; and the traversals per
sample r, with SE from the spread of the chunk values of both renders
(2 x (CHUNKS - 1) degrees of freedom pooled into one normal-theory bound),

    |rA - rR| <= 7 SE + allowance rR.

"se > 0" is read at the precision of the mode under test: a channel whose
samples are all one value in exact arithmetic (the sky's blue channel is 1, so
a pixel of ground under it is 0.5) comes out of the fp32 mode with the jitter
of single-precision rounding, se / m around 1e-9, and a difference from the
fp64 mean of the same kind, 5e-8 m: dozens of such "standard errors" that
measure rounding, not sampling.  So a channel counts as without variance
where sqrt(seA^2 + seR^2) <= 2^-24 max(|mA|, |mR|), a single-precision unit
roundoff of its mean.  The three scale rules above are applied to it as they
stand, with its se as computed; only the z-scores (the rms, the largest z
reported) leave it out, and an excess is reported as "zero_variance".

The multipliers are normal-tail bounds for the number of comparisons a suite
makes: about 1e5 pixel channels (2 Phi(-6) = 2e-9 each), 7e3 blocks (2 Phi(-5)
= 6e-7), a few dozen frames (2 Phi(-4) = 6e-5) and traversal counts (t with 15
degrees of freedom beyond 7: 4e-6), each below 1e-2 over the whole suite.

Power is a separate matter (`NoPower`, neither a pass nor a failure): on the
reference alone the frame term 4 sqrt(sum seR^2) / npix must be at most
1e-3 level, and the median seR / m over channels with m > 0.01 level at most
0.5 %.  The control compares two seeds of the reference through the same
function with allowance 0.
"""
from dataclasses import dataclass, field

import numpy as np

CHUNKS = 16
ALLOWANCE = 1e-3       # floor / level, and the traversal count's relative term
Z_PIXEL, Z_BLOCK, Z_FRAME, Z_TRAVERSALS = 6.0, 5.0, 4.0, 7.0
BLOCK = 4
RMS_MAX = 1.1
RESOLUTION = 2.0 ** -24  # se / m at or below single precision's unit roundoff: no sampling variance
POWER_FRAME = 1e-3     # 4 sqrt(sum seR^2) / npix <= POWER_FRAME * level
POWER_MEDIAN = 5e-3    # median seR / m
POWER_MIN_M = 1e-2     # ... over channels with m > POWER_MIN_M * level


class NoPower(Exception):
    """The reference render is too noisy for the comparison to mean anything:
    more samples (or a quieter scene) are needed."""


@dataclass
class Render:
    S1: np.ndarray          # nx*ny*3 sums
    S2: np.ndarray          # nx*ny*3 sums of squares
    n: int                  # samples per pixel
    segments: list          # traversals of each chunk
    samples: list           # samples of each chunk


@dataclass
class Result:
    failures: list = field(default_factory=list)   # names of the rules broken
    max_pixel_z: float = 0.0
    max_block_z: float = 0.0
    frame_z: float = 0.0     # the largest of the three channels', signed
    z_rms: float = 0.0
    rel_frame_diff: float = 0.0   # (sum mA - sum mR) / sum mR over all channels, no floor
    traversals: tuple = (0.0, 0.0)  # per sample: A, R
    traversals_z: float = 0.0
    detail: list = field(default_factory=list)

    def row(self) -> str:
        return (f"pixel z {self.max_pixel_z:5.2f}  block z {self.max_block_z:5.2f}  frame z {self.frame_z:+5.2f}  "
                f"z rms {self.z_rms:5.3f}  frame diff {self.rel_frame_diff:+.2e}  "
                f"trav/sample {self.traversals[0]:.4f} vs {self.traversals[1]:.4f} (z {self.traversals_z:+5.2f})")


def mean_and_se2(r: Render):
    """(m, se^2) of every channel."""
    n = float(r.n)
    if r.n < 2:
        raise ValueError("a standard error needs two samples")
    m = r.S1 / n
    se2 = np.maximum(r.S2 - r.S1 * m, 0.0) / ((n - 1.0) * n)
    return m, se2


def level_of(ref: Render) -> float:
    return float(mean_and_se2(ref)[0].mean())


def power(ref: Render, nx: int, ny: int) -> dict:
    """The power condition's two figures on the reference alone (relative to
    the level): raises NoPower where either is over its cap."""
    m, se2 = mean_and_se2(ref)
    level = float(m.mean())
    if not level > 0:
        raise NoPower("the reference frame is black")
    frame = float((4.0 * np.sqrt(se2.reshape(-1, 3).sum(axis=0)) / (nx * ny)).max() / level)
    lit = m > POWER_MIN_M * level
    median = float(np.median(np.sqrt(se2[lit]) / m[lit]))
    out = {"frame_term": frame, "median_rel_se": median, "level": level}
    if frame > POWER_FRAME or median > POWER_MEDIAN:
        raise NoPower(f"no power: frame term {frame:.2e} of the level (cap {POWER_FRAME:.0e}), "
                      f"median se/m {median:.2e} (cap {POWER_MEDIAN:.0e}) at {ref.n} samples per pixel")
    return out


def _traversals(r: Render):
    per = np.asarray(r.segments, dtype=np.float64) / np.asarray(r.samples, dtype=np.float64)
    rate = float(np.sum(r.segments) / np.sum(r.samples))
    return rate, float(per.var(ddof=1) / per.size)


def compare(A: Render, R: Render, nx: int, ny: int, allowance: float = ALLOWANCE) -> Result:
    """Every rule of the module's docstring on A against R; the broken ones by
    name in Result.failures ("pixel", "zero_variance", "block", "frame", "rms",
    "traversals").  No pixel is left out of any rule."""
    if nx % BLOCK or ny % BLOCK:
        raise ValueError(f"the image must tile into {BLOCK}x{BLOCK} blocks")
    if len(A.segments) != CHUNKS or len(R.segments) != CHUNKS:
        raise ValueError(f"a render is taken in {CHUNKS} chunks")
    mA, vA = mean_and_se2(A)
    mR, vR = mean_and_se2(R)
    if not (np.all(np.isfinite(mA)) and np.all(np.isfinite(vA)) and np.all(np.isfinite(mR)) and np.all(np.isfinite(vR))):
        raise ValueError("non-finite moments")
    npix = nx * ny
    floor = allowance * float(mR.mean())
    d = (mA - mR).reshape(ny, nx, 3)
    v = (vA + vR).reshape(ny, nx, 3)
    s = np.sqrt(v)
    res = Result()

    # pixels
    over = np.abs(d) > Z_PIXEL * s + floor
    flat = s <= RESOLUTION * np.maximum(np.abs(mA), np.abs(mR)).reshape(ny, nx, 3)
    if np.any(over & ~flat):
        res.failures.append("pixel")
    if np.any(over & flat):
        res.failures.append("zero_variance")
    z = np.divide(d, s, out=np.zeros_like(d), where=~flat)
    if np.any(~flat):
        res.max_pixel_z = float(np.abs(z[~flat]).max())
        res.z_rms = float(np.sqrt(np.mean(z[~flat] ** 2)))
    if res.z_rms >= RMS_MAX:
        res.failures.append("rms")
    for j, i, c in np.argwhere(over)[:8]:
        res.detail.append(f"pixel ({i},{j}) channel {c}: diff {d[j, i, c]:+.4e}, se {s[j, i, c]:.3e}, floor {floor:.3e}")

    # 4x4 blocks
    def tiles(a):
        return a.reshape(ny // BLOCK, BLOCK, nx // BLOCK, BLOCK, 3).sum(axis=(1, 3))
    db, sb = tiles(d), np.sqrt(tiles(v))
    over_b = np.abs(db) > Z_BLOCK * sb + BLOCK * BLOCK * floor
    if np.any(over_b):
        res.failures.append("block")
    noisy = sb > RESOLUTION * tiles(np.maximum(np.abs(mA), np.abs(mR)).reshape(ny, nx, 3))
    if np.any(noisy):
        res.max_block_z = float(np.abs(db[noisy] / sb[noisy]).max())
    for j, i, c in np.argwhere(over_b)[:8]:
        res.detail.append(f"block ({i},{j}) channel {c}: diff {db[j, i, c]:+.4e}, se {sb[j, i, c]:.3e}")

    # the frame
    df, sf = d.sum(axis=(0, 1)), np.sqrt(v.sum(axis=(0, 1)))
    if np.any(np.abs(df) > Z_FRAME * sf + npix * floor):
        res.failures.append("frame")
        res.detail.append(f"frame: diff {df / npix}, se {sf / npix}, floor {floor:.3e}")
    zf = np.divide(df, sf, out=np.zeros(3), where=sf > 0)
    res.frame_z = float(zf[np.argmax(np.abs(zf))])
    res.rel_frame_diff = float(d.sum() / mR.sum()) if mR.sum() != 0 else 0.0

    # traversals per sample
    rA, varA = _traversals(A)
    rR, varR = _traversals(R)
    se = float(np.sqrt(varA + varR))
    res.traversals = (rA, rR)
    res.traversals_z = (rA - rR) / se if se > 0 else 0.0
    if abs(rA - rR) > Z_TRAVERSALS * se + allowance * rR:
        res.failures.append("traversals")
        res.detail.append(f"traversals per sample {rA:.6f} vs {rR:.6f}, se {se:.2e}")
    return res


def assert_same(A: Render, R: Render, nx: int, ny: int, allowance: float = ALLOWANCE, what: str = "") -> Result:
    """compare(), after the power condition on R; fails with the broken rules."""
    power(R, nx, ny)
    res = compare(A, R, nx, ny, allowance)
    assert not res.failures, f"{what}: {res.failures}: {res.row()}\n  " + "\n  ".join(res.detail)
    return res
