"""GPU tier: every GEMM of a small matrix of one-step adaptations takes the kernel, tile, grid, split count and epilogue
it took before the dispatcher computed a route (csrc/gemm.hip gemm_route).

tests/golden/g17_gemm_census_parent.json holds the GEMM census of each run of tests/golden/record_gemm_census.py's
matrix (defaults in the three precisions, each routing switch at its off and forced settings, ragged pairs and
batch-64 grids that reach the 256 x 256 kernels' thresholds), recorded on an MI355X with the library of the commit
before the route; the census of the same run on this library must equal it exactly, keys and counts.
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("record_gemm_census", os.path.join(GOLDEN, "record_gemm_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
with open(REC.FIXTURE) as _f:
    RECORDED = json.load(_f)


def test_recording_holds_every_run_and_every_reachable_family():
    assert sorted(RECORDED) == sorted(r["name"] for r in REC.RUNS)
    REC.check_coverage(RECORDED)


@pytest.mark.parametrize("run", REC.RUNS, ids=[r["name"] for r in REC.RUNS])
def test_gemm_census_equals_the_parent_commits(monkeypatch, run):
    census = REC.run_census(run, setenv=monkeypatch.setenv, delenv=lambda k: monkeypatch.delenv(k, raising=False))
    want = RECORDED[run["name"]]
    diff = {k: (want.get(k), census.get(k)) for k in sorted(set(want) | set(census)) if want.get(k) != census.get(k)}
    assert not diff, "census entry: (recorded, now)\n" + "\n".join(f"{k}: {v}" for k, v in diff.items())
