"""Radiance queries (include/rtw_radiance.h), CPU side: the header and ABI
table, rtw_radiance_params of _abi.py against the header's sizeof / offsetof,
the host layer (csrc/host/radiance.cpp: every refusal that needs no device, the
chunk / pass / staging plan) and the ray-sourced kernel choice (rtw_select.h
select_rays) through tests/cpp/radiance_check.cpp, built plainly and with
-fsanitize=address,undefined as a program of its own, and the oracle
tests/cpp/host_radiance.cpp on cases whose answer is known without a GPU.  No
GPU compute here."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from raytracingweekend_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "raytracingweekend_amd"
CSRC = PKG / "csrc"
HOST = CSRC / "host"
HEADER = ROOT / "include" / "rtw_radiance.h"

FLAVOURS = {"plain": ["-O1"],
            "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                          "-O1"]}


def _radiance_check(tmp_path, flavour):
    inc = [f"-I{ROOT / 'include'}", f"-I{CSRC}", f"-I{HOST}"]
    exe = tmp_path / "radiance_check"
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", *FLAVOURS[flavour], *inc,
           str(ROOT / "tests" / "cpp" / "radiance_check.cpp"),
           *[str(HOST / s) for s in ("radiance.cpp", "render_plan.cpp", "noise.cpp", "output.cpp")], "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "OK (radiance_check)", (r.stdout + r.stderr)[-4000:]
    return r.stdout


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_radiance_host_code(tmp_path, flavour):
    """Every refusal of rtw_radiance_check_args; rtw_radiance_plan at n = 0, 1,
    n * spp = 2^32 - 1 and 2^32, 2^32 - 1 rays and with small bounds: the chunks
    tile [0, n) once with their first_key offsets, no pass above the 32-bit id
    or the budget, staged chunks within the byte bound; select_rays over the
    selection grid."""
    out = _radiance_check(tmp_path, flavour)
    for n in (0, 1, 1000, 1431655765, 2**30, 2**32 - 1):
        assert f"plan n={n} " in out
    assert "plan n=1431655765 spp=3 staged=0 rng=0: 1 chunks of 1431655765, 1 passes walked" in out
    assert "plan n=1073741824 spp=4 staged=0 rng=0: 1 chunks of 1073741824, 2 passes walked" in out


def test_selection_of_ray_sourced_kernels(tmp_path):
    """The four built-in defaults get their persistent row (no F_PIN: 256 is
    not in the feature word), everything else k_regen_rays + a wavefront form;
    all three kinds occur on the grid."""
    out = _radiance_check(tmp_path, "plain")
    want = {"cornell_box": "k_persist_sort<1136, 8, true>", "random_balls": "k_persist_sort<1160, 12, false>",
            "random_balls/bvh": "k_persist<1154, 12, false, true>", "book2_final/bvh": "k_persist<1125, 29, false, true>"}
    got = dict(l[len("scene "):].split(": ", 1) for l in out.splitlines() if l.startswith("scene "))
    assert got == want
    for name in want.values():
        f = int(re.search(r"<(\d+),", name).group(1))
        assert f & 1024 and not f & 256 and not f & 512
    kinds = {l.rsplit(": ", 1)[0]: int(l.rsplit(": ", 1)[1]) for l in out.splitlines()
             if l.startswith(("persistent row", "k_regen_rays + "))}
    assert set(kinds) == {"persistent row", "k_regen_rays + k_segment", "k_regen_rays + split pair"}
    assert all(v > 0 for v in kinds.values()) and sum(kinds.values()) == 6 * 55296


def test_struct_matches_the_header(tmp_path):
    out = _radiance_check(tmp_path, "plain")
    cls = _abi.rtw_radiance_params
    line = next(l for l in out.splitlines() if l.startswith(f"sizeof {cls.__name__} "))
    words = line.split()
    assert int(words[2]) == C.sizeof(cls) == 40, line
    got = dict(zip(words[3::2], map(int, words[4::2])))
    assert got == {name: getattr(cls, name).offset for name, _ in cls._fields_}, line


def test_header_adds_symbols_only_and_the_abi_table_has_them(built):
    text = HEADER.read_text()
    names = set(re.findall(r"\b(rtw_[a-z_]+)\s*\(", text.split("#ifndef RTW_RADIANCE_H")[1]))
    assert names == set(_abi.RADIANCE_SIGNATURES), names ^ set(_abi.RADIANCE_SIGNATURES)
    assert '#include "rtw_query.h"' in text
    assert _abi.RTW_ABI_VERSION == 4 and _abi.lib().rtw_abi_version() == 4
    for lib in ("librtw.so", "_build/librtw_strict.so"):
        nm = subprocess.run(["nm", "-D", "--defined-only", str(PKG / lib)], capture_output=True, text=True).stdout
        for name in _abi.RADIANCE_SIGNATURES:
            assert f" T {name}\n" in nm, (lib, name)


def test_refusals_before_any_device(built):
    """Through the library, with a handle that is never read: the device-free
    refusals come first."""
    L = _abi.lib()
    rays, sums = np.zeros((2, 8)), np.zeros((2, 3))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    prm = _abi.rtw_radiance_params(max_depth=5, spp_count=1)
    assert L.rtw_trace_radiance(None, p(rays), 2, None, C.byref(prm), p(sums), None) == -1
    assert b"null scene handle" in L.rtw_last_error()
    fake = C.c_int(0)
    h = C.cast(C.byref(fake), C.c_void_p)
    assert L.rtw_trace_radiance(h, p(rays), 2, None, None, p(sums), None) == -1
    for bad in (dict(spp_count=0), dict(spp_count=1, spp_begin=-1), dict(spp_count=1, max_depth=-1),
                dict(spp_count=1, first_key=2**32 - 1)):
        prm = _abi.rtw_radiance_params(**{"max_depth": 5, **bad})
        assert L.rtw_trace_radiance(h, p(rays), 2, None, C.byref(prm), p(sums), None) == -1, bad
    prm = _abi.rtw_radiance_params(max_depth=5, spp_count=2)
    rng = np.ones(2, dtype=np.uint32)
    assert L.rtw_trace_radiance(h, p(rays), 2, p(rng), C.byref(prm), p(sums), None) == -1
    prm = _abi.rtw_radiance_params(max_depth=5, spp_count=1, precision=1)
    assert L.rtw_trace_radiance(h, p(rays), 2, None, C.byref(prm), p(sums), None) == -5
    prm = _abi.rtw_radiance_params(max_depth=5, spp_count=1)
    assert L.rtw_trace_radiance(h, p(rays), 2, None, C.byref(prm), p(rays), None) == -1
    assert b"overlap" in L.rtw_last_error()
    assert L.rtw_trace_radiance(h, None, 0, None, C.byref(prm), None, None) == 0  # n == 0: a no-op
    assert L.rtw_scene_query_radiance(None, C.create_string_buffer(128)) == -1
    assert not sums.any()


def test_cli_refuses_bad_radiance_options(built):
    """Decided from the arguments alone, before any device is touched."""
    cli = PKG / "rtw_render"
    for opts in (["--radiance", "s.bin"], ["--rays", "r.bin", "--radiance", "s.bin", "--hits", "h.bin"],
                 ["--rays", "r.bin", "--radiance", "s.bin", "--occluded"],
                 ["--rays", "r.bin", "--radiance", "s.bin", "--out", "x.ppm"],
                 ["--rays", "r.bin", "--radiance", "s.bin", "--gpus", "2"],
                 ["--rays", "r.bin", "--radiance", "s.bin", "--precision", "fp32"],
                 ["--rays", "r.bin", "--radiance", "s.bin", "--spp", "0"]):
        r = subprocess.run([str(cli), *opts], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--radiance FILE --spp N" in r.stderr and "in fp64, without --hits" in r.stderr, \
            (opts, r.stdout, r.stderr)


# ---- the oracle on the CPU ---------------------------------------------------------------
def _pixel_centre_rays(sd, nx, ny):
    """The desc camera's rays through the pixel centres, lens radius 0
    (camera.h get_ray with rd = 0), at the shutter's opening."""
    c = sd.camera
    o, ll = np.array(c.origin[:]), np.array(c.lower_left[:])
    hz, vt = np.array(c.horizontal[:]), np.array(c.vertical[:])
    j, i = np.mgrid[0:ny, 0:nx]
    u, v = ((i + 0.5) / nx).ravel(), ((j + 0.5) / ny).ravel()
    rays = np.empty((nx * ny, 8))
    rays[:, :3] = o
    rays[:, 3:6] = ll + u[:, None] * hz + v[:, None] * vt - o
    rays[:, 6], rays[:, 7] = c.time0, np.inf
    return rays


def test_host_radiance_oracle(built, tmp_path):
    """tests/cpp/host_radiance.cpp on cornell_box's pixel-centre camera rays:
    two runs give the same bytes; depth 0 gives zero sums and no traversal;
    Normal mode draws nothing, so every sample of a ray is one traversal with
    one value v and three samples sum to (v + v) + v exactly; keyed streams
    differ from sample to sample and from key to key in colour mode."""
    from test_gpu_denoise import _compile
    from raytracingweekend_amd import render
    exe = _compile("host_radiance.cpp", tmp_path / "host_radiance")
    rays = _pixel_centre_rays(render.SceneDesc("cornell_box", 1.0), 8, 8)
    rays.tofile(tmp_path / "rays.bin")
    n = len(rays)

    def run(scene, begin, count, depth, seed, key, tag, rng="-"):
        out = tmp_path / f"{tag}.bin"
        r = subprocess.run([str(exe), scene, str(tmp_path / "rays.bin"), rng, str(begin), str(count), str(depth),
                            str(seed), str(key), str(out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        raw = np.fromfile(out, dtype=np.uint8)
        return raw[:n * 24].view(np.float64).reshape(n, 3), int(raw[n * 24:].view(np.uint64)[0])

    a, ta = run("cornell_box", 2, 3, 50, 11, 100, "a")
    b, tb = run("cornell_box", 2, 3, 50, 11, 100, "b")
    assert np.array_equal(a, b, equal_nan=True) and ta == tb and ta >= 3 * n and a.any()
    z, tz = run("cornell_box", 2, 3, 0, 11, 100, "z")
    assert not z.any() and tz == 0
    one, t1 = run("normal:cornell_box", 0, 1, 50, 11, 0, "n1")
    three, t3 = run("normal:cornell_box", 5, 3, 50, 99, 7, "n3")
    assert t1 == n and t3 == 3 * n
    assert np.array_equal(three, (one + one) + one) and one.any()
    # keys and samples: single samples add up to the range's sums, other keys give other paths
    parts = [run("cornell_box", s, 1, 50, 11, 100, f"s{s}")[0] for s in (2, 3, 4)]
    assert np.array_equal(a, (parts[0] + parts[1]) + parts[2])
    other, _ = run("cornell_box", 2, 3, 50, 11, 101, "k")
    assert not np.array_equal(a, other)
    # given states: a state a keyed stream starts from reproduces that sample
    L = _abi.lib()
    states = np.array([L.rtw_path_seed(11, 100 + k, 2) for k in range(n)], dtype=np.uint32)
    states.tofile(tmp_path / "rng.bin")
    given, _ = run("cornell_box", 0, 1, 50, 0, 0, "g", rng=str(tmp_path / "rng.bin"))
    assert np.array_equal(given, parts[0])
