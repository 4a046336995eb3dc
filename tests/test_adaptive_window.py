"""The window rule of adaptive sampling (include/rtw_adaptive_window.h), CPU
side: the header and ABI table, the host select against a numpy restatement of
the definition and on hand-built images, its equality with the plain select at
radius 0, the refusals, and the host code under AddressSanitizer / UBSan
(tests/cpp/adaptive_window_check.cpp, a program of its own: nothing is
preloaded).  No GPU compute here; tests/test_gpu_adaptive_window.py runs the
same cases (random_case, hand_cases) through the device select."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from raytracingweekend_amd import _abi
from test_adaptive import MAX_COUNT, moments, rel_np
from test_noise import FLOOR

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "raytracingweekend_amd" / "csrc"
HOST = CSRC / "host"
HEADER = ROOT / "include" / "rtw_adaptive_window.h"
SIZES = [(1, 1), (5, 3), (63, 4), (64, 4), (65, 4), (130, 9), (300, 7)]
RADII = [0, 1, 2, 16]


def source_np(s1, s2, counts, target_rel, floor=FLOOR):
    """SOURCE of rtw_adaptive_window.h: finite, and counts < 2 or rel > target_rel."""
    rel, _, fin = rel_np(s1, s2, counts, floor)
    with np.errstate(invalid="ignore"):
        return fin & ((counts < 2) | (rel > target_rel)), fin


def window_np(s1, s2, counts, nx, ny, target_rel, min_count, max_count, radius, floor=FLOOR):
    """The definition: ELIGIBLE and a SOURCE in the clipped window, the window
    as ORs of shifted slices (no wrap, no mirror)."""
    src, fin = source_np(s1, s2, counts, target_rel, floor)
    src = src.reshape(ny, nx)
    near = np.zeros_like(src)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if abs(dy) >= ny or abs(dx) >= nx:
                continue
            # near[j, i] |= src[j + dy, i + dx] where both lie inside the image
            j0, j1 = max(0, -dy), min(ny, ny - dy)
            i0, i1 = max(0, -dx), min(nx, nx - dx)
            near[j0:j1, i0:i1] |= src[j0 + dy:j1 + dy, i0 + dx:i1 + dx]
    on = fin & (counts >= min_count) & (counts < max_count) & near.reshape(-1)
    return np.flatnonzero(on).astype(np.uint32)


_cases = {}


def random_case(nx, ny):
    """test_adaptive.moments of the size (NaN / Inf pixels, counts 0, 1, 2 and
    at / above MAX_COUNT among them) and a target_rel -- a quantile of the
    finite rel values -- under which between 1 % and 10 % of the pixels are
    sources: with most pixels sources every list is "all eligible pixels" and
    shows nothing.  The pixels with fewer than two samples are sources under
    any target (about 8 % of `moments`' pixels), so the quantile is taken such
    that the judged sources fill half of what is left below 10 %, at least one;
    the first seed of `moments` for which that fits is used.  A one-pixel
    image has a share of 0 or 1: its target makes the pixel a source if it can
    be one, and the share is not asserted."""
    if (nx, ny) in _cases:
        return _cases[nx, ny]
    npix = nx * ny
    for seed in range(64):
        s1, s2, counts = moments(nx, ny, seed)
        rel, _, fin = rel_np(s1, s2, counts)
        always = int((fin & (counts < 2)).sum())
        judged = np.sort(rel[fin & (counts >= 2)])[::-1]  # loudest first; a source whatever its count
        k = max(1, (npix // 10 - always) // 2)
        if npix == 1:
            target = float(judged[0]) / 2 if judged.size else 0.1
            break
        if judged.size > k and judged[k] < judged[k - 1] and 0.01 * npix <= always + k <= 0.10 * npix:
            target = float(judged[k])  # rel > target: exactly the k loudest
            break
    else:
        raise AssertionError(f"no seed of moments({nx}, {ny}) gives a share of sources in [1 %, 10 %]")
    src, _ = source_np(s1, s2, counts, target)
    _cases[nx, ny] = dict(s1=s1, s2=s2, counts=counts, target=target, share=float(src.mean()), seed=seed)
    return _cases[nx, ny]


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("nx,ny", SIZES)
def test_host_select_matches_the_definition(built, nx, ny, radius):
    from raytracingweekend_amd import render
    c = random_case(nx, ny)
    if nx * ny > 1:
        assert 0.01 <= c["share"] <= 0.10, c["share"]
    sizes = []
    for min_count in (0, 3):
        want = window_np(c["s1"], c["s2"], c["counts"], nx, ny, c["target"], min_count, MAX_COUNT, radius)
        got = render.select_active_window(c["s1"], c["s2"], c["counts"], nx, ny, target_rel=c["target"],
                                          max_count=MAX_COUNT, min_count=min_count, radius=radius, floor=FLOOR)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (nx, ny, radius, min_count, got.size, want.size)
        sizes.append(got.size)
    assert sizes[1] <= sizes[0]
    if nx * ny >= 63 * 4:
        # the lists show something: neither empty nor every eligible pixel, and
        # min_count takes pixels away
        _, fin = source_np(c["s1"], c["s2"], c["counts"], c["target"])
        eligible = int((fin & (c["counts"] < MAX_COUNT)).sum())
        assert 0 < sizes[1] < sizes[0] and (sizes[0] < eligible or radius == 16), (sizes, eligible)


@pytest.mark.parametrize("nx,ny", SIZES)
def test_radius_0_is_the_plain_select(built, nx, ny):
    from raytracingweekend_amd import render
    c = random_case(nx, ny)
    for target in (c["target"], 0.0, 1e9):
        plain = render.select_active(c["s1"], c["s2"], c["counts"], nx, ny, target_rel=target, max_count=MAX_COUNT,
                                     floor=FLOOR)
        win = render.select_active_window(c["s1"], c["s2"], c["counts"], nx, ny, target_rel=target,
                                          max_count=MAX_COUNT, min_count=0, radius=0, floor=FLOOR)
        assert np.array_equal(plain, win), (nx, ny, target)


# ---- hand-built images --------------------------------------------------------------
HAND = dict(nx=130, ny=9, radius=2, min_count=4, max_count=8, target=0.1)
LOUD = ([4.0, 4.0, 4.0], [40.0, 40.0, 40.0])  # four samples with spread: rel ~ 0.6


def quiet(nx, ny, n):
    """Every pixel n equal samples of 0.5: variance 0, rel 0, nobody a source."""
    return np.full(nx * ny * 3, 0.5 * n), np.full(nx * ny * 3, 0.25 * n), np.full(nx * ny, n, dtype=np.uint32)


def square(nx, ny, i, j, r):
    """The pixels of the window of (i, j), clipped to the image, ascending."""
    jj, ii = np.mgrid[max(0, j - r):min(ny, j + r + 1), max(0, i - r):min(nx, i + r + 1)]
    return np.sort((jj * nx + ii).reshape(-1)).astype(np.uint32)


def hand_cases():
    """(name, s1, s2, counts, expected list) on quiet moments with all counts
    at min_count; HAND has the other arguments."""
    nx, ny, r, n = HAND["nx"], HAND["ny"], HAND["radius"], HAND["min_count"]
    out = []

    def loud(s1, s2, p):
        s1[3 * p:3 * p + 3], s2[3 * p:3 * p + 3] = LOUD

    spots = {"corner (0, 0)": (0, 0), "corner (nx-1, 0)": (nx - 1, 0), "corner (0, ny-1)": (0, ny - 1),
             "corner (nx-1, ny-1)": (nx - 1, ny - 1), "i = 63": (63, 4), "i = 64": (64, 4),
             "the last column": (nx - 1, 4)}
    for name, (i, j) in spots.items():
        s1, s2, counts = quiet(nx, ny, n)
        loud(s1, s2, j * nx + i)
        out.append((f"one source, {name}", s1, s2, counts, square(nx, ny, i, j, r)))
    i, j = 64, 4
    p = j * nx + i
    sq = square(nx, ny, i, j, r)
    # a NaN pixel inside the square is not listed ...
    s1, s2, counts = quiet(nx, ny, n)
    loud(s1, s2, p)
    s1[3 * (p + 1) + 1] = np.nan
    out.append(("a NaN pixel in the square", s1, s2, counts, sq[sq != p + 1]))
    # ... and is no source: alone it lists nobody
    s1, s2, counts = quiet(nx, ny, n)
    s1[3 * p] = np.nan
    out.append(("a NaN pixel alone", s1, s2, counts, np.zeros(0, np.uint32)))
    s1, s2, counts = quiet(nx, ny, n)
    s2[3 * p + 2] = np.inf
    out.append(("an Inf pixel alone", s1, s2, counts, np.zeros(0, np.uint32)))
    # a pixel with fewer than two samples is a source (and, below min_count, not listed itself)
    s1, s2, counts = quiet(nx, ny, n)
    counts[p] = 1
    out.append(("a pixel with one sample", s1, s2, counts, sq[sq != p]))
    # a loud pixel at max_count is not listed but lists its neighbours
    s1, s2, counts = quiet(nx, ny, n)
    loud(s1, s2, p)
    counts[p] = HAND["max_count"]
    s1[3 * p:3 * p + 3], s2[3 * p:3 * p + 3] = [8.0] * 3, [80.0] * 3  # eight samples, the same spread
    out.append(("a source at max_count", s1, s2, counts, sq[sq != p]))
    # a pixel below min_count inside the square is not listed
    s1, s2, counts = quiet(nx, ny, n)
    loud(s1, s2, p)
    counts[p - nx - 2] = n - 1
    s1[3 * (p - nx - 2):3 * (p - nx - 2) + 3] = 0.5 * (n - 1)
    s2[3 * (p - nx - 2):3 * (p - nx - 2) + 3] = 0.25 * (n - 1)
    out.append(("a pixel below min_count in the square", s1, s2, counts, sq[sq != p - nx - 2]))
    # two sources whose squares overlap across the word boundary: the union, once
    s1, s2, counts = quiet(nx, ny, n)
    loud(s1, s2, 4 * nx + 62)
    loud(s1, s2, 5 * nx + 65)
    out.append(("two sources across i = 63 | 64", s1, s2, counts,
                np.union1d(square(nx, ny, 62, 4, r), square(nx, ny, 65, 5, r)).astype(np.uint32)))
    return out


def test_hand_built_images(built):
    from raytracingweekend_amd import render
    nx, ny = HAND["nx"], HAND["ny"]
    for name, s1, s2, counts, want in hand_cases():
        got = render.select_active_window(s1, s2, counts, nx, ny, target_rel=HAND["target"], floor=FLOOR,
                                          min_count=HAND["min_count"], max_count=HAND["max_count"],
                                          radius=HAND["radius"])
        assert np.array_equal(got, want), (name, got, want)
        # the numpy restatement reads the cases the same way
        assert np.array_equal(want, window_np(s1, s2, counts, nx, ny, HAND["target"], HAND["min_count"],
                                              HAND["max_count"], HAND["radius"])), name
    # the square's sizes: 3x3 in a corner, 5x5 inside, 3x5 at the last column
    sizes = [c[4].size for c in hand_cases()[:7]]
    assert sizes == [9, 9, 9, 9, 25, 25, 15], sizes


def test_refusals(built):
    from raytracingweekend_amd import render
    lib = _abi.lib()
    s1, s2, counts = quiet(2, 2, 4)
    out = np.zeros(4, np.uint32)
    n = C.c_uint64()
    p1, p2, pc, po = (x.ctypes.data_as(C.c_void_p) for x in (s1, s2, counts, out))

    def call(a=p1, q=p2, c=pc, nx=2, ny=2, floor=FLOOR, target=0.1, lo=0, hi=8, radius=1, o=po, nn=C.byref(n)):
        return lib.rtw_adaptive_select_window(a, q, c, nx, ny, floor, target, lo, hi, radius, o, nn)

    assert call() == 0 and n.value == 0
    assert call(lo=8, hi=8) == 0, "min_count == max_count is an empty range, not an error"
    for kw, word in (({"radius": -1}, "radius"), ({"radius": _abi.RTW_WINDOW_RADIUS_MAX + 1}, "radius"),
                     ({"lo": 9, "hi": 8}, "min_count"), ({"a": None}, "null"), ({"c": None}, "null"),
                     ({"o": None}, "null"), ({"nn": None}, "null"), ({"nx": 0}, "size"), ({"ny": -1}, "size"),
                     ({"floor": 0.0}, "floor"), ({"floor": float("nan")}, "floor"), ({"target": -0.5}, "target_rel"),
                     ({"target": float("nan")}, "target_rel"), ({"q": p1}, "overlap"), ({"o": pc}, "overlap")):
        assert call(**kw) == -1, kw
        msg = lib.rtw_last_error().decode()
        assert "rtw_adaptive_select_window" in msg and word in msg, (kw, msg)
    with pytest.raises(_abi.RtwError, match="radius"):
        render.select_active_window(s1, s2, counts, 2, 2, target_rel=0.1, max_count=8, radius=17)
    # the device entry points decide the same from the arguments alone: no scene is touched
    assert lib.rtw_adaptive_select_window_device(None, p1, p2, pc, 2, 2, FLOOR, 0.1, 0, 8, 1, po, C.byref(n)) == -1
    assert b"rtw_adaptive_select_window_device" in lib.rtw_last_error()
    assert lib.rtw_render_adaptive_window(None, None, None, None, 0, None, None, None, None, None) == -1
    assert b"rtw_render_adaptive_window" in lib.rtw_last_error()
    ap = _abi.rtw_adaptive_params(target_rel=0.1, floor=FLOOR, min_spp=4, max_spp=8, batch=0)
    for radius in (-1, 17):
        assert lib.rtw_render_adaptive_window(None, None, None, C.byref(ap), radius, None, None, None, None, None) == -1
        assert b"radius" in lib.rtw_last_error()
    for kw in ({"window": -1}, {"window": 17}, {"window": 2, "min_spp": 1}):
        with pytest.raises(ValueError):
            render.render_adaptive(None, 8, 8, 64, 50, **{"target_rel": 0.1, **kw})


def declared_functions():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(rtw_[a-z_0-9]+)\s*\(", text)))


def test_header_and_abi_table(built, tmp_path):
    from raytracingweekend_amd import build
    names = declared_functions()
    assert names == ["rtw_adaptive_select_window", "rtw_adaptive_select_window_device", "rtw_render_adaptive_window"]
    assert names == sorted(_abi.ADAPTIVE_WINDOW_SIGNATURES)
    others = (set(_abi.SIGNATURES) | set(_abi.NOISE_SIGNATURES) | set(_abi.ADAPTIVE_SIGNATURES) |
              set(_abi.DENOISE_SIGNATURES))
    assert not set(names) & others
    lib = _abi.lib()
    if not build.STRICT_LIB.exists():
        pytest.fail(f"{build.STRICT_LIB} is missing: run `python -m raytracingweekend_amd.build` first")
    for path in (_abi.LIB_PATH, build.STRICT_LIB):
        nm = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
        for n in names:
            assert re.search(rf"\bT {n}$", nm, re.M), f"{n} is not a defined text symbol of {path.name}"
    assert all(hasattr(lib, n) for n in names)
    text = " ".join(re.sub(r"^ \*", "", HEADER.read_text(), flags=re.M).split())  # (without the comment's margin)
    assert f"#define RTW_WINDOW_RADIUS_MAX {_abi.RTW_WINDOW_RADIUS_MAX}" in text
    assert '#include "rtw_adaptive.h"' in text
    # the bias note and the invariant are part of the interface
    assert "BIAS." in text and "REDUCES the bias, it does not remove it" in text
    assert "never comes back" in text and "clipped at the borders" in text
    # the header is C11 and adds no struct; the ABI version is the library's
    src = tmp_path / "c11.c"
    src.write_text('#include "rtw_adaptive_window.h"\n'
                   "int main(void){ return RTW_WINDOW_RADIUS_MAX == 16 && RTW_ABI_VERSION == %d ? 0 : 1; }\n"
                   % _abi.RTW_ABI_VERSION)
    exe = tmp_path / "c11"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


FLAVOURS = {"plain": ["-O1"],
            "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                          "-O1"]}


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_window_host_code(tmp_path, flavour):
    """tests/cpp/adaptive_window_check.cpp over adaptive_window.cpp and
    adaptive.cpp: the hand-built cases, radius 16 on a 5x3 image, random images
    against the definition spelt out there, the plain select at radius 0 and
    the refusals; built plainly and with -fsanitize=address,undefined and run
    directly."""
    inc = [f"-I{ROOT / 'include'}", f"-I{CSRC}", f"-I{HOST}"]
    exe = tmp_path / "adaptive_window_check"
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", *FLAVOURS[flavour], *inc,
           str(ROOT / "tests" / "cpp" / "adaptive_window_check.cpp"),
           *[str(HOST / s) for s in ("adaptive_window.cpp", "adaptive.cpp", "noise.cpp", "output.cpp")], "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "OK (adaptive_window_check)", (r.stdout + r.stderr)[-4000:]


def test_cli_refuses_bad_window_options(built):
    """Decided from the arguments alone, before any device is touched."""
    cli = ROOT / "raytracingweekend_amd" / "rtw_render"
    for opts in (["--adaptive-window", "2"], ["--adaptive", "0.1", "--adaptive-window", "-1"],
                 ["--adaptive", "0.1", "--adaptive-window", "17"], ["--noise", "--adaptive-window", "1"]):
        p = subprocess.run([str(cli), *opts], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "--adaptive-window needs --adaptive" in p.stderr, (opts, p.stdout, p.stderr)
