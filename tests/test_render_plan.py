"""The plan of a render call (csrc/host/render_plan.cpp) on the CPU:
tests/cpp/render_plan_check.cpp built with g++ -ffp-contract=off from the host
sources it needs, once plainly and once with -fsanitize=address,undefined (a
program with its own main; any sanitizer report fails the run).

a. Same plan as before it became a function of its own.
   tests/golden/render_plan_parent.json holds, for every call of
   tests/cpp/render_plan_cases.h, what the commit before render_plan.cpp
   existed made of it: the refusal's code and text, or the no-op's sample
   count, or spp_count, row_step, n_rows, npix, the pool and pass sizes, the
   bytes of every buffer it ensured, the hit records' split, the device camera
   and the fp32 camera bit for bit, the job's fields and, per pass, total,
   spp_pass, div_spp, s_begin and the wavefront form's fill and iteration cap.
   It was recorded from that commit's render_accumulate: its refusals, sizing,
   ensures, carving, camera, job and pass-loop lines verbatim (with job_t,
   carve_paths / carve_fresh and host_splitmix64), compiled in a host-only
   harness whose dev_buf::ensure records its argument and whose HIP calls do
   nothing, built once plainly and once with RTW_STRICT_RADIANCE=1 for the
   strict case.  It is never regenerated from render_plan.cpp.
   The refusals: nx = 0, spp = 0, spp_begin > spp, spp_count < 0, a range past
   spp, precision 7, row_begin -1 and ny, 65536 x 65536, 46341 x 46341, a
   moving-sphere BVH with the shutter outside the build's, overlapping moment
   buffers.  Sizing: 8 x 8 x 8 spp from sample 5 with budget 192 (passes of 3,
   3, 2), a budget below npix, wavefront_paths 0 / 1000 / above pass_samples,
   rows 1, 3 of 5, 4096 x 4096 x 1024 spp with budget 2^40 (pass_spp 255).
b. `render_plan_check check`: the three dividers equal udiv_magic of their
   divisors; sample_coords' arithmetic restated on the host gives the right
   (i, j, s) for the first, the last and 1 000 spread ids of every pass; the
   cameras (thin lens unchanged, lens-less with u[1] = inf: NaN lens_radius,
   the same with lens_radius 0.1 unchanged, cam32 = the (float) casts, dtime =
   (float)(time1 - time0)); a no-op sizes nothing; for caps 1, 1000 and 2^21
   every carved array lies inside its pool, none overlap, the last ends at the
   pool's end; rtw_render_multi's two messages from the shared range check."""
import json
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "raytracingweekend_amd" / "csrc"
HOST = CSRC / "host"
SOURCES = ["render_plan.cpp", "noise.cpp", "output.cpp"]
FLAVOURS = {"plain": ["-O1"],
            "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                          "-O1"]}
ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
REFUSALS = {
    "nx_zero": "rtw_render_accumulate: bad image / sample parameters",
    "spp_zero": "rtw_render_accumulate: bad image / sample parameters",
    "begin_past_spp": "rtw_render_accumulate: bad image / sample parameters",
    "count_negative": "rtw_render_accumulate: bad image / sample parameters",
    "range_past_spp": "sample range exceeds spp",
    "precision_7": "rtw_render_accumulate: unknown precision",
    "row_begin_minus1": "row_begin out of range",
    "row_begin_ny": "row_begin out of range",
    "image_65536": "image too large for 32-bit pixel ids",
    "image_46341": "image too large for 32-bit pixel ids",
    "shutter_outside": "rtw_render_accumulate: camera shutter outside the one the scene's BVH was built for "
                       "(moving spheres); flatten the scene with this camera",
    "moments_overlap": "rtw_render_accumulate_moments: accum_rgb and accum_sq_rgb overlap",
}


@pytest.fixture(scope="module", params=list(FLAVOURS))
def program(request, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("render_plan_check_" + request.param)
    inc = [f"-I{ROOT / 'include'}", f"-I{CSRC}", f"-I{HOST}", f"-I{ROOT / 'tests' / 'cpp'}"]
    exe = tmp / "render_plan_check"
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", *FLAVOURS[request.param], *inc,
           str(ROOT / "tests" / "cpp" / "render_plan_check.cpp"), *[str(HOST / s) for s in SOURCES], "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run(exe, mode):
    r = subprocess.run([str(exe), mode], capture_output=True, text=True, timeout=300, env={**os.environ, **ENV})
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return r.stdout


def test_plan_equals_the_parents_render_accumulate(program):
    want = json.loads((ROOT / "tests" / "golden" / "render_plan_parent.json").read_text())["cases"]
    got = {}
    for line in run(program, "dump").splitlines():
        row = json.loads(line)
        got[row.pop("name")] = row
    assert sorted(got) == sorted(want) and len(want) == 34
    for name in want:
        g, w = got[name], want[name]
        assert g == w, (name, {k: (g.get(k), w.get(k)) for k in set(g) | set(w) if g.get(k) != w.get(k)})
    # the recording holds what this test says it does
    for name, text in REFUSALS.items():
        assert want[name] == {"rc": -1, "error": text}, name
    assert want["begin_equals_spp"] == {"rc": 0, "noop": 1, "samples": 0}
    assert want["depth_zero"] == {"rc": 0, "noop": 1, "samples": 3 * 64}
    p = want["passes_3_3_2"]["passes"]
    assert [(x["spp_pass"], x["total"], x["s_begin"]) for x in p] == [(3, 192, 5), (3, 192, 8), (2, 128, 11)]
    b = want["budget_below_npix"]
    assert b["pass_spp"] == 1 and [x["spp_pass"] for x in b["passes"]] == [1, 1, 1]
    assert [want[n]["pool"] for n in ("paths_default", "paths_1000", "paths_above_pass")] == [16384, 1000, 256]
    assert (want["rows_1_step_2"]["n_rows"], want["rows_1_step_2"]["npix"]) == (2, 14)
    c = want["pass_cap_2_32"]
    assert c["pass_spp"] == 255 and all(x["total"] < 2 ** 32 for x in c["passes"]) and len(c["passes"]) == 5
    assert want["strict_256_cus"]["flog_threads"] == 256 * 2048


def test_plan_properties(program):
    out = run(program, "check")
    assert out.splitlines()[-1] == "OK (17 planned calls)", out[-4000:]
