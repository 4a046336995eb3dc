"""Ray queries (include/rtw_query.h), CPU side: the header and ABI table, the
three structs of _abi.py against the header's sizeof / offsetof, and the host
layer (csrc/host/query.cpp: every refusal that needs no device, the launch and
staging plan) through tests/cpp/query_check.cpp, built plainly and with
-fsanitize=address,undefined as a program of its own.  No GPU compute here."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from raytracingweekend_amd import _abi

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "raytracingweekend_amd" / "csrc"
HOST = CSRC / "host"
HEADER = ROOT / "include" / "rtw_query.h"

FLAVOURS = {"plain": ["-O1"],
            "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                          "-O1"]}


def _query_check(tmp_path, flavour):
    inc = [f"-I{ROOT / 'include'}", f"-I{CSRC}", f"-I{HOST}"]
    exe = tmp_path / "query_check"
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", *FLAVOURS[flavour], *inc,
           str(ROOT / "tests" / "cpp" / "query_check.cpp"), *[str(HOST / s) for s in ("query.cpp", "output.cpp")],
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "OK (query_check)", (r.stdout + r.stderr)[-4000:]
    return r.stdout


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_query_host_code(tmp_path, flavour):
    """Every refusal of rtw_query_check_args and rtw_query_check_camera_args;
    rtw_query_plan at n = 0, 1, 2^31 - 1, 2^31, 2^32 + 5 and with small bounds:
    the launches tile [0, n) exactly once, none above the 32-bit limit, staged
    chunks within the byte bound."""
    out = _query_check(tmp_path, flavour)
    for n in (0, 1, 2**31 - 1, 2**31, 2**32 + 5):
        assert f"plan n={n} " in out


def test_structs_match_the_header(tmp_path):
    """sizeof and offsetof of rtw_query_ray, rtw_query_hit and rtw_query_params
    as the C compiler lays the header out, against _abi.py and the numpy record
    of render.py."""
    out = _query_check(tmp_path, "plain")
    for cls in (_abi.rtw_query_ray, _abi.rtw_query_hit, _abi.rtw_query_params):
        line = next(l for l in out.splitlines() if l.startswith(f"sizeof {cls.__name__} "))
        words = line.split()
        assert int(words[2]) == C.sizeof(cls), line
        got = dict(zip(words[3::2], map(int, words[4::2])))
        assert got == {name: getattr(cls, name).offset for name, _ in cls._fields_}, line
    assert C.sizeof(_abi.rtw_query_ray) == 64 and C.sizeof(_abi.rtw_query_hit) == 64
    assert C.sizeof(_abi.rtw_query_params) == 16
    from raytracingweekend_amd.render import QUERY_HIT_DTYPE
    assert QUERY_HIT_DTYPE.itemsize == 64
    assert {k: v[1] for k, v in QUERY_HIT_DTYPE.fields.items()} == \
        {name: getattr(_abi.rtw_query_hit, name).offset for name, _ in _abi.rtw_query_hit._fields_}


def test_header_adds_symbols_only_and_the_abi_table_has_them(built):
    text = HEADER.read_text()
    names = set(re.findall(r"\b(rtw_[a-z_]+)\s*\(", text.split("#ifndef RTW_QUERY_H")[1]))
    assert names == set(_abi.QUERY_SIGNATURES), names ^ set(_abi.QUERY_SIGNATURES)
    assert _abi.RTW_ABI_VERSION == 4 and _abi.lib().rtw_abi_version() == 4
    assert "#define RTW_ABI_VERSION 4" in (ROOT / "include" / "rtw_gpu.h").read_text()
    for lib in ("librtw.so", "_build/librtw_strict.so"):
        nm = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "raytracingweekend_amd" / lib)],
                            capture_output=True, text=True).stdout
        for name in _abi.QUERY_SIGNATURES:
            assert f" T {name}\n" in nm, (lib, name)


def test_null_arguments_are_refused_before_any_device(built):
    """The refusals that need neither a handle nor a GPU, through the library."""
    L = _abi.lib()
    prm = _abi.rtw_query_params()
    rays = np.zeros((2, 8))
    hits = np.zeros((2, 8))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.rtw_trace_closest(None, p(rays), 2, None, C.byref(prm), p(hits), None) == -1
    assert b"null scene handle" in L.rtw_last_error()
    assert L.rtw_trace_occluded(None, p(rays), 0, None, C.byref(prm), p(hits), None) == -1
    a, b = C.create_string_buffer(128), C.create_string_buffer(128)
    assert L.rtw_scene_query_trace(None, a, b) == -1
    assert L.rtw_camera_rays(None, None, None, p(rays), None, 2) == -1


def test_cli_refuses_bad_query_options(built):
    """Decided from the arguments alone, before any device is touched."""
    cli = ROOT / "raytracingweekend_amd" / "rtw_render"
    for opts in (["--rays", "r.bin"], ["--hits", "h.bin"], ["--occluded"], ["--rng", "g.bin"],
                 ["--rays", "r.bin", "--hits", "h.bin", "--gpus", "2"],
                 ["--rays", "r.bin", "--hits", "h.bin", "--denoise"]):
        p = subprocess.run([str(cli), *opts], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "--rays" in p.stderr, (opts, p.stdout, p.stderr)
