"""rtw_scene_query on the MI355X: the kernels, node packet and LDS bytes it
reports for every scene of tests/golden/scene_*.json, flat and with BVHs,
under RTW_MODE / RTW_SPLIT (this process) and RTW_SORT (child processes),
equal tests/golden/scene_query_gfx950.json -- scripts/record_scene_query.py's
output before kernel selection moved to rtw_select.h.  Scenes are uploaded,
nothing is rendered."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def recorder(built):
    from raytracingweekend_amd import render
    if render.device_count() < 1:
        pytest.fail("no GPU visible to the HIP runtime")
    spec = importlib.util.spec_from_file_location("record_scene_query", ROOT / "scripts" / "record_scene_query.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_scene_query_equals_the_recorded_answers(recorder):
    want = json.loads((ROOT / "tests" / "golden" / "scene_query_gfx950.json").read_text())
    got = recorder.record()
    assert sorted(got) == sorted(want)
    for env in sorted(want):
        assert sorted(got[env]) == sorted(want[env]), env
        for scene in sorted(want[env]):
            assert got[env][scene] == want[env][scene], (env, scene)
