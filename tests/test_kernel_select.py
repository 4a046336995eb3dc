"""Kernel selection (csrc/rtw_select.h) on the CPU: tests/cpp/select_check.cpp
walks select_fp64 / select_fp32 over the grids of
tests/golden/kernel_selection.json -- the names the launch probes gave before
selection became a function of its own -- and every row must be equal.  The
program also fails when a choice has no entry in the instantiation lists the
launch tables are built from; for a split choice (k_intersect + k_shade), when
the rows split_resolve gives are not listed or are not the instantiations the
launch switches named before the pair came from the tables (their case labels
and default rows, written out in the program)."""
import json
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "raytracingweekend_amd" / "csrc"
KEYS = {"fp64": ("unset", "0", "1"), "fp32": ("unset", "0")}


def test_selection_equals_the_recorded_probes(tmp_path):
    exe = tmp_path / "select_check"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", f"-I{CSRC}", str(ROOT / "tests" / "cpp" / "select_check.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("# "):
            rows = got.setdefault(tuple(line[2:].split()), [])
        else:
            rows.append(line)
    gold = json.loads((ROOT / "tests" / "golden" / "kernel_selection.json").read_text())
    blocks = [(p, b, k) for p in ("fp64", "fp32") for b in ("default", "strict") for k in KEYS[p]]
    assert sorted(got) == sorted(blocks)
    for p, b, k in blocks:
        rows = "".join(gold["chunks"][p][i] for i in gold[p][b][k])
        want = [gold["names"][p][gold["alphabet"].index(c)] for c in rows]
        assert len(got[p, b, k]) == len(want) == (55296 if p == "fp64" else 512)
        diff = [(i, g, w) for i, (g, w) in enumerate(zip(got[p, b, k], want)) if g != w]
        assert not diff, f"{p} {b} {k}: {len(diff)} rows differ, first (row, got, want): {diff[:5]}"
