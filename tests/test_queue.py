"""The sharded sample queue's arithmetic (csrc/rtw_queue.h) on the CPU:
tests/cpp/queue_check.cpp built with g++, once plainly and once with
-fsanitize=address,undefined (a program with its own main; any sanitizer
report fails the run).  For the totals 0, 1, 63, 64, 65, 1023, 1024, 1025,
8191, 8192, 8193, 8200, 9216, 9217, 25*1024+5 and 100 000: the shards' limits
sum to the total, the shards' samples are each id of [0, total) exactly once,
and queue_drained is false with any one shard one short of its limit and true
at the limits."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "raytracingweekend_amd" / "csrc"
FLAVOURS = {"plain": ["-O1"],
            "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                          "-O1"]}
ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
TOTALS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 8200, 9216, 9217, 25 * 1024 + 5, 100000]


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_queue_shards_cover_every_sample_once(flavour, tmp_path):
    exe = tmp_path / "queue_check"
    cmd = ["g++", "-std=c++17", "-Wall", *FLAVOURS[flavour], f"-I{CSRC}", str(ROOT / "tests" / "cpp" / "queue_check.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env={**os.environ, **ENV})
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == f"OK ({len(TOTALS)} totals)", r.stdout[-4000:]
    # the program checked the totals this test names
    assert lines[:-1] == [f"total {t}: limits sum {t}" for t in TOTALS]
