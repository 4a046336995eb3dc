"""Adaptive per-pixel sampling (include/rtw_adaptive.h), CPU side: the header
and ABI table, the host select / estimate / finalize with counts against numpy,
the loop's schedule, kernel selection of an active render
(tests/cpp/select_active_check.cpp), the plan of an active call and the host
code under AddressSanitizer / UBSan (tests/cpp/adaptive_check.cpp, a program of
its own: nothing is preloaded).  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from raytracingweekend_amd import _abi
from test_noise import FLOOR, noise_np, same_bits

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "raytracingweekend_amd" / "csrc"
HOST = CSRC / "host"
HEADER = ROOT / "include" / "rtw_adaptive.h"
SIZES = [(1, 1), (300, 7), (600, 500)]
MAX_COUNT = 64


def rel_np(s1, s2, counts, floor=FLOOR):
    """rtw_noise.h's rel_p with n = counts[p], verbatim, and the finite mask."""
    s1 = np.asarray(s1, dtype=np.float64).reshape(-1, 3)
    s2 = np.asarray(s2, dtype=np.float64).reshape(-1, 3)
    dn = counts.astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        m = s1 / dn
        v = (s2 - s1 * m) / (dn - 1.0)
        v = np.where(v < 0, 0.0, v)
        se = np.sqrt(v / dn)
        rel = ((se[:, 0] + se[:, 1]) + se[:, 2]) / (((m[:, 0] + m[:, 1]) + m[:, 2]) + 3 * np.float64(floor))
    fin = np.isfinite(s1).all(axis=1) & np.isfinite(s2).all(axis=1)
    return rel, se, fin


def active_np(s1, s2, counts, target_rel, max_count, floor=FLOOR):
    """The definition of rtw_adaptive.h: counts < max_count, finite moments,
    and counts < 2 or rel > target_rel."""
    rel, _, fin = rel_np(s1, s2, counts, floor)
    with np.errstate(invalid="ignore"):
        on = (counts < max_count) & fin & ((counts < 2) | (rel > target_rel))
    return np.flatnonzero(on).astype(np.uint32)


def moments(nx, ny, seed=0):
    """Random raw moments with counts 0, 1, 2, MAX_COUNT - 1, MAX_COUNT and
    above among them, and NaN / Inf pixels."""
    npix = nx * ny
    rng = np.random.default_rng([seed, nx, ny])
    counts = rng.integers(2, MAX_COUNT, npix).astype(np.uint32)
    special = rng.random(npix) < 0.25
    counts[special] = rng.choice([0, 1, 2, MAX_COUNT - 1, MAX_COUNT, MAX_COUNT + 3], int(special.sum()))
    mean = rng.random((npix, 1)) * 2.0
    spread = rng.random((npix, 1)) * rng.random((npix, 1))
    s1 = np.zeros((npix, 3))
    s2 = np.zeros((npix, 3))
    for k in range(MAX_COUNT + 3):
        x = mean + spread * (rng.random((npix, 3)) - 0.5)
        live = (k < counts)[:, None]
        s1 = np.where(live, s1 + x, s1)
        s2 = np.where(live, s2 + x * x, s2)
    if npix > 10:
        bad = rng.choice(npix, max(2, npix // 90), replace=False)
        s1[bad[::2], 1] = np.nan
        s2[bad[1::2], 0] = np.inf
    return s1.reshape(-1), s2.reshape(-1), counts


@pytest.mark.parametrize("nx,ny", SIZES)
def test_host_select_matches_the_definition(built, nx, ny):
    from raytracingweekend_amd import render
    s1, s2, counts = moments(nx, ny)
    rel, _, fin = rel_np(s1, s2, counts)
    judged = fin & (counts >= 2) & (counts < MAX_COUNT)
    half = float(np.median(rel[judged])) if judged.any() else 0.02
    seen = []
    for target in (1e9, 0.0, half):
        got = render.select_active(s1, s2, counts, nx, ny, target_rel=target, max_count=MAX_COUNT, floor=FLOOR)
        want = active_np(s1, s2, counts, target, MAX_COUNT)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (nx, ny, target, got.size, want.size)
        assert (np.diff(got.astype(np.int64)) > 0).all(), "the list must be strictly ascending"
        seen.append(got.size)
    if nx * ny > 1:
        # none but the pixels without a variance yet; all the judged ones with spread; about half
        assert seen[0] == int((fin & (counts < 2)).sum()) > 0
        assert seen[1] > 0.9 * int((fin & (counts < MAX_COUNT)).sum())
        assert 0.35 * judged.sum() < seen[2] - seen[0] < 0.65 * judged.sum(), seen
    # pixels at or above max_count, and NaN / Inf pixels, are never active
    all_on = render.select_active(s1, s2, counts, nx, ny, target_rel=0.0, max_count=MAX_COUNT, floor=FLOOR)
    assert not (counts[all_on] >= MAX_COUNT).any() and fin[all_on].all()


def test_select_edge_pixels(built):
    """Single pixels: no samples, one sample, at max_count, NaN with no
    samples, a constant pixel (rel == 0 is not above a target of 0)."""
    from raytracingweekend_amd import render

    def on(s1, s2, n, target=0.1):
        return render.select_active(np.array(s1, dtype=float), np.array(s2, dtype=float), np.array([n], np.uint32), 1, 1,
                                    target_rel=target, max_count=8, floor=FLOOR).size == 1

    assert on([0, 0, 0], [0, 0, 0], 0) and on([1, 1, 1], [1, 1, 1], 1)
    assert not on([1, 1, 1], [9, 9, 9], 8) and not on([1, 1, 1], [9, 9, 9], 9)
    assert not on([np.nan, 0, 0], [0, 0, 0], 0) and not on([1, 1, 1], [np.inf, 1, 1], 4)
    assert on([4, 4, 4], [40, 40, 40], 4) and not on([4, 4, 4], [40, 40, 40], 4, target=1e9)
    assert not on([2, 2, 2], [2, 2, 2], 2, target=0.0), "a constant pixel has rel == 0"


@pytest.mark.parametrize("n", [2, 7, 64])
def test_uniform_counts_equal_the_uniform_functions(built, n):
    from raytracingweekend_amd import render
    nx, ny = 37, 11
    s1, s2, _ = moments(nx, ny, seed=n)
    counts = np.full(nx * ny, n, dtype=np.uint32)
    se_u, sum_u = render.noise_estimate(s1, s2, nx, ny, n, FLOOR)
    se_c, sum_c = render.noise_estimate_counts(s1, s2, counts, nx, ny, FLOOR)
    assert same_bits(se_u, se_c) and sum_u == sum_c
    assert sum_c["nonfinite"] > 0, "the case holds non-finite pixels"
    with np.errstate(all="ignore"):
        assert same_bits(render.finalize(s1, nx, ny, n), render.finalize_counts(s1, counts, nx, ny))


def test_mixed_counts_match_numpy(built):
    from raytracingweekend_amd import render
    nx, ny = 300, 7
    s1, s2, counts = moments(nx, ny, seed=3)
    se, summ = render.noise_estimate_counts(s1, s2, counts, nx, ny, FLOOR)
    rel, se_np, fin = rel_np(s1, s2, counts)
    keep = fin & (counts >= 2)
    want_se = np.where(keep[:, None], se_np, np.nan).reshape(-1)
    assert same_bits(se, want_se)
    k = int(keep.sum())
    assert summ["pixels"] == k and summ["nonfinite"] == nx * ny - k and (counts < 2).any()
    assert summ["mean_rel"] == pytest.approx(float(rel[keep].sum() / k), rel=1e-12)
    assert summ["max_rel"] == float(rel[keep].max())
    assert summ["rms_stderr"] == pytest.approx(float(np.sqrt((se_np[keep] ** 2).sum() / (k * 3.0))), rel=1e-12)
    # the uniform estimator's numpy model agrees where a pixel's count is the uniform one
    se7, _ = noise_np(s1, s2, 7)
    at7 = np.repeat(keep & (counts == 7), 3)
    assert at7.any() and np.array_equal(se[at7], se7[at7])
    with np.errstate(all="ignore"):
        canvas = render.finalize_counts(s1, counts, nx, ny)
        # (np.minimum passes a NaN through, as the library's `1.0 < s ? 1.0 : s` does)
        want = np.minimum(np.sqrt(s1.reshape(-1, 3) / counts.astype(np.float64)[:, None]), 1.0).reshape(-1)
    assert same_bits(canvas, want) and np.isnan(canvas).any()


def test_schedule(built):
    from raytracingweekend_amd import render
    assert render.adaptive_schedule(8, 32, 8) == [(0, 8), (8, 8), (16, 8), (24, 8)]
    assert render.adaptive_schedule(8, 50, 0) == [(0, 8), (8, 8), (16, 16), (32, 18)]
    assert render.adaptive_schedule(16, 16, 0) == [(0, 16)] == render.adaptive_schedule(16, 16, 5)
    assert render.adaptive_schedule(2, 9, 4) == [(0, 2), (2, 4), (6, 3)]
    assert render.adaptive_schedule(8, 11, 0) == [(0, 8), (8, 3)]
    lib = _abi.lib()
    ap = _abi.rtw_adaptive_params(target_rel=0.1, floor=FLOOR, min_spp=8, max_spp=32, batch=8)
    b, c = C.c_int(), C.c_int()
    assert lib.rtw_adaptive_next_round(C.byref(ap), 32, C.byref(b), C.byref(c)) == 0 and c.value == 0
    for done in (3, 33, -1):
        assert lib.rtw_adaptive_next_round(C.byref(ap), done, C.byref(b), C.byref(c)) == -1
        assert b"done" in lib.rtw_last_error()


def test_render_adaptive_argument_errors(built):
    """Decided from the arguments alone: no scene is touched."""
    from raytracingweekend_amd import render
    for kw in ({"min_spp": 1}, {"max_spp": 7}, {"batch": -1}, {"target_rel": -0.1}, {"target_rel": float("nan")},
               {"floor": 0.0}, {"precision": "fp16"}):
        args = {"max_spp": 64, "target_rel": 0.1, "min_spp": 8, "batch": 0, "floor": FLOOR, **kw}
        with pytest.raises(ValueError):
            render.render_adaptive(None, 8, 8, args.pop("max_spp"), 50, **args)
    lib = _abi.lib()
    assert lib.rtw_render_adaptive(None, None, None, None, None, None, None, None, None) == -1
    assert b"rtw_render_adaptive" in lib.rtw_last_error()
    assert lib.rtw_render_accumulate_active(None, None, None, None, 0, None, None, None, None) == -1
    assert b"rtw_render_accumulate_active" in lib.rtw_last_error()
    name = C.create_string_buffer(128)
    assert lib.rtw_scene_query_active(None, 0, name) == -1
    a = np.ones(12)
    c = np.ones(4, dtype=np.uint32)
    n = C.c_uint64()
    pa, pc = a.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)
    assert lib.rtw_adaptive_select_device(None, pa, pa, pc, 2, 2, FLOOR, 0.1, 8, pc, C.byref(n)) == -1
    assert lib.rtw_noise_estimate_counts_device(None, pa, pa, pc, 2, 2, FLOOR, None, None) == -1
    assert lib.rtw_finalize_canvas_counts_device(None, pa, pc, 2, 2, pa) == -1


def declared_functions():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(rtw_[a-z_0-9]+)\s*\(", text)))


def test_header_and_abi_table(built, tmp_path):
    from raytracingweekend_amd import build
    names = declared_functions()
    assert names == sorted(_abi.ADAPTIVE_SIGNATURES) and len(names) == 10
    assert not set(names) & (set(_abi.SIGNATURES) | set(_abi.NOISE_SIGNATURES))
    lib = _abi.lib()
    if not build.STRICT_LIB.exists():
        pytest.fail(f"{build.STRICT_LIB} is missing: run `python -m raytracingweekend_amd.build` first")
    for path in (_abi.LIB_PATH, build.STRICT_LIB):
        nm = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True).stdout
        for n in names:
            assert re.search(rf"\bT {n}$", nm, re.M), f"{n} is not a defined text symbol of {path.name}"
    assert all(hasattr(lib, n) for n in names)
    # the bias note is part of the interface
    text = " ".join(HEADER.read_text().split())
    assert "biases dark, heavy-tailed pixels LOW" in text and "min_spp exists" in text
    # the header is C11, and the structs' layouts are the ctypes mirrors'
    structs = {"rtw_adaptive_params": (_abi.rtw_adaptive_params, 32), "rtw_adaptive_result": (_abi.rtw_adaptive_result, 64)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rtw_adaptive.h"', "int main(void){"]
    for s, (mirror, _) in structs.items():
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        for f, _ in mirror._fields_:
            lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = dict(l.rsplit(" ", 1) for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.split("\n") if l)
    for s, (mirror, size) in structs.items():
        assert int(out[s]) == C.sizeof(mirror) == size, s
        for f, _ in mirror._fields_:
            assert int(out[f"{s}.{f}"]) == getattr(mirror, f).offset, (s, f)


def test_active_selection_is_always_instantiated(tmp_path):
    exe = tmp_path / "select_active_check"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", f"-I{CSRC}",
                        str(ROOT / "tests" / "cpp" / "select_active_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "OK", (r.stdout + r.stderr)[-3000:]
    rows = dict(l.split(": ", 1) for l in r.stdout.splitlines() if ": " in l)
    # the built-in scenes run their own kernels with the bit (F_ACTIVE = 512) ...
    assert rows["scene cornell_box"] == "k_persist_sort<624, 8, true> | k_fast_sort<4608, true>"
    assert rows["scene random_balls"] == "k_persist_sort<648, 12, false> | k_fast_sort<4608, false>"
    assert rows["scene random_balls/bvh"] == "k_persist<642, 12, false, true> | k_fast<4610, true>"
    assert rows["scene book2_final/bvh"] == "k_persist<869, 29, false, true> | k_fast<517, true>"
    # ... and every kind of choice occurs on the grids
    for kind in ("fp64 persistent", "fp64 k_regen_active + k_segment", "fp64 k_regen_active + split pair",
                 "fp32 the whole-image kernel with the bit", "fp32 general k_fast of the walk",
                 "fp32 refused (image textures)"):
        assert int(rows[kind]) > 0, kind
    assert sum(int(rows[k]) for k in rows if k.startswith("fp64")) == 6 * 55296
    assert sum(int(rows[k]) for k in rows if k.startswith("fp32")) == 2 * 512


FLAVOURS = {"plain": ["-O1"],
            "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                          "-O1"]}


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_adaptive_host_code_and_active_plan(tmp_path, flavour):
    """tests/cpp/adaptive_check.cpp over adaptive.cpp and render_plan.cpp: the
    host select, estimate and finalize with counts, the list check, the
    schedule and the plan of an active call; built plainly and with
    -fsanitize=address,undefined and run directly."""
    inc = [f"-I{ROOT / 'include'}", f"-I{CSRC}", f"-I{HOST}"]
    exe = tmp_path / "adaptive_check"
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", *FLAVOURS[flavour], *inc,
           str(ROOT / "tests" / "cpp" / "adaptive_check.cpp"),
           *[str(HOST / s) for s in ("adaptive.cpp", "render_plan.cpp", "noise.cpp", "output.cpp")], "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "OK (adaptive_check)", (r.stdout + r.stderr)[-4000:]


def test_cli_refuses_bad_adaptive_options(built):
    """Decided from the arguments alone, before any device is touched."""
    cli = ROOT / "raytracingweekend_amd" / "rtw_render"
    for opts, word in ((["--adaptive", "0.1", "--gpus", "2"], "one GPU"), (["--adaptive", "0.1", "--noise"], "one GPU"),
                       (["--adaptive", "-1"], "target >= 0"), (["--adaptive", "0.1", "--min-spp", "1"], "--min-spp >= 2"),
                       (["--adaptive", "0.1", "--spp", "8"], "--spp >= --min-spp"),
                       (["--adaptive", "0.1", "--noise-batch", "0"], "--noise-batch >= 1"),
                       (["--adaptive", "0.1", "--noise-floor", "0"], "--noise-floor > 0")):
        p = subprocess.run([str(cli), *opts], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and word in p.stderr, (opts, p.stdout, p.stderr)
