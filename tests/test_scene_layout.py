"""The device scene layout (csrc/host/scene_layout.cpp) on the CPU:
tests/cpp/layout_check.cpp built with g++ -ffp-contract=off from the host
sources it needs, once plainly and once with -fsanitize=address,undefined
(a program with its own main; any sanitizer report fails the run).

a. Same bytes as before the layout became a function of its own.
   tests/golden/scene_layout_parent.json holds, for every scene of
   tests/golden/scene_*.json but the probe scenes, `ties` and the `textured` image scene, flat and with
   BVHs: the SHA-256 of the two blobs, every array's offset (-1: a null
   pointer), every scalar of scene / fscene and every fact.  It was recorded
   from the commit before this file existed: that commit's upload_scene, its
   body verbatim, compiled in a host-only harness whose handle allocates with
   malloc and whose hipMemcpy is memcpy, dumping scene_mem, scene32 and the
   handle's fields after each upload.  It is never regenerated from
   scene_layout.cpp.
b. Selection end to end: select_in filled from the layout's facts with the
   desc's own camera, through select_fp64 / select_fp32 under the five
   environments of scripts/record_scene_query.py, gives the kernel,
   kernel_fast and shade_lds_bytes of tests/golden/scene_query_gfx950.json
   (bvh_lds_nodes needs an occupancy query: tests/test_gpu_scene_query.py).
c. Hand-built descs, the smallest at which each step can go wrong
   (`layout_check cases`)."""
import hashlib
import json
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "raytracingweekend_amd" / "csrc"
HOST = CSRC / "host"
GOLDEN = ROOT / "tests" / "golden"
SOURCES = ["scene_layout.cpp", "flatten.cpp", "scene_api.cpp", "scenes.cpp", "output.cpp", "validate.cpp",
           "image_io.cpp"]
FLAVOURS = {"plain": ["-O1"],
            "sanitized": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g",
                          "-O1"]}
ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}


@pytest.fixture(scope="module", params=list(FLAVOURS))
def program(request, tmp_path_factory):
    """layout_check of one flavour, and what `layout_check scenes` gave:
    (exe, {scene: json}, {scene: {blob: bytes}})."""
    tmp = tmp_path_factory.mktemp("layout_check_" + request.param)
    inc = [f"-I{ROOT / 'include'}", f"-I{CSRC}", f"-I{HOST}", f"-I{HOST / 'rtw'}"]
    exe = tmp / "layout_check"
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", *FLAVOURS[request.param], *inc,
           str(ROOT / "tests" / "cpp" / "layout_check.cpp"), *[str(HOST / s) for s in SOURCES], "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = tmp / "blobs"
    out.mkdir()
    r = subprocess.run([str(exe), "scenes", str(out)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, **ENV})
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    rows, blobs = {}, {}
    for line in r.stdout.splitlines():
        key, doc = line.split("\t")
        rows[key] = json.loads(doc)
        blobs[key] = {m: (out / f"{key.replace('/', '_')}.{m}").read_bytes() for m in ("mem64", "mem32")}
    return exe, rows, blobs


def test_layout_equals_the_parents_upload(program):
    _, rows, blobs = program
    want = json.loads((GOLDEN / "scene_layout_parent.json").read_text())
    # (the probe scenes' dumps and the ties scene's are younger than the parent's upload: not among its scenes)
    scenes = [p.stem[len("scene_"):] for p in sorted(GOLDEN.glob("scene_*.json"))
              if "aspect" in json.loads(p.read_text()) and not p.stem.startswith("scene_probe_")
              and p.stem != "scene_ties"]
    assert len(scenes) == 7
    assert sorted(want) == sorted(f"{s}/{v}" for s in scenes + ["textured"] for v in ("flat", "bvh"))
    assert sorted(rows) == sorted(want)
    for key in sorted(want):
        got, w = rows[key], want[key]
        for m in ("mem64", "mem32"):
            assert len(blobs[key][m]) == w[m + "_bytes"] == got["off" + m[3:]]["end"], (key, m)
            assert hashlib.sha256(blobs[key][m]).hexdigest() == w[m + "_sha256"], (key, m)
        for part in ("off64", "off32", "scalars", "facts"):
            g = {k: v for k, v in got[part].items() if k not in ("end", "_")}
            assert g == w[part], (key, part, {k: (g.get(k), w[part].get(k)) for k in set(g) | set(w[part])
                                              if g.get(k) != w[part].get(k)})


def test_selection_from_the_layout_equals_the_recorded_queries(program):
    _, rows, _ = program
    want = json.loads((GOLDEN / "scene_query_gfx950.json").read_text())
    assert sorted(want) == ["default", "sort0", "sort1", "wavefront", "wavefront_split"]
    for env in want:
        assert len(want[env]) == 14
        for scene in sorted(want[env]):
            w = {k: want[env][scene][k] for k in ("kernel", "kernel_fast", "shade_lds_bytes")}
            assert rows[scene]["select"][env] == w, (env, scene)


def test_hand_built_scenes(program):
    exe, _, _ = program
    r = subprocess.run([str(exe), "cases"], capture_output=True, text=True, timeout=300, env={**os.environ, **ENV})
    assert r.returncode == 0 and r.stdout.startswith("OK ("), (r.stdout + r.stderr)[-4000:]
