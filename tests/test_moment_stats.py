"""The per-pixel moment statistics (csrc/host/moments.h) through the public
entry points: the bits recorded from the library before the arithmetic was
folded into one header (tests/golden/moment_stats_parent.json, written by
scripts/record_moment_stats.py), on the host and on the card; and the header
alone under AddressSanitizer / UBSan (tests/cpp/moments_check.cpp, a program
of its own: nothing is preloaded)."""
import os
import subprocess
from pathlib import Path

import pytest

import moment_stats

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "raytracingweekend_amd" / "csrc"


def assert_recorded(got: dict, want: dict):
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name]["inputs"] == want[name]["inputs"], f"{name}: the input generator drifted, not the library"
        diff = [k for k in want[name] if got[name].get(k) != want[name][k]]
        assert not diff and sorted(got[name]) == sorted(want[name]), (name, diff)


def test_host_bits_are_the_recorded_ones(built):
    from raytracingweekend_amd import render
    assert_recorded(moment_stats.record(render, device=False), moment_stats.golden("host"))


@pytest.mark.gpu
def test_device_bits_are_the_recorded_ones(built):
    """The device summaries against the device's own record (its fold order is
    not the host's)."""
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    assert_recorded(moment_stats.record(render, device=True), moment_stats.golden("device"))


def test_moments_header_is_sanitizer_clean(tmp_path):
    exe = tmp_path / "moments_check"
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", f"-I{ROOT / 'include'}",
                        f"-I{CSRC}", f"-I{CSRC / 'host'}", str(ROOT / "tests" / "cpp" / "moments_check.cpp"), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
           "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "OK (moments_check)", (r.stdout + r.stderr)[-4000:]
