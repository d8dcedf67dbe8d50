"""Every LayerNorm launch computes bitwise what it computed before the launches were described by LnSite and chosen by
ln_fwd_route / ln_bwd_route (csrc/norm.h).

tests/golden/g18_ln_parent.npz holds, for each run of tests/golden/record_ln_baseline.py's matrix (every scalar and
vectorised width, the fused conv backward on both sides of its chunk-size switch, the bf16 plane forms at their
defaults and with each switch alone, the positional stack, a frozen feature encoder, biases only), the logits of
steps 0 and 2 of a two-step adaptation and the sha256 of every adapted tensor, recorded on an MI355X with the library
of the commit before the routes; the same run on this library must reproduce both exactly.
"""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("record_ln_baseline", os.path.join(GOLDEN, "record_ln_baseline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
RECORDED = np.load(REC.FIXTURE)


def test_recording_holds_every_run_and_the_matrix_every_launch_class():
    assert sorted({k.split("/")[0] for k in RECORDED.files}) == sorted(r["name"] for r in REC.RUNS)
    REC.check_coverage(REC.RUNS)


@pytest.mark.gpu
@pytest.mark.parametrize("run", REC.RUNS, ids=[r["name"] for r in REC.RUNS])
def test_layernorm_launches_are_bitwise_the_parent_commits(monkeypatch, run):
    got = REC.run(run, setenv=monkeypatch.setenv, delenv=lambda k: monkeypatch.delenv(k, raising=False))
    name = run["name"]
    assert got["weights_sha256"] == str(RECORDED[name + "/weights_sha256"]), "the seeded weights changed"
    assert np.array_equal(got["logits"], RECORDED[name + "/logits"])
    assert got["params_sha256"] == str(RECORDED[name + "/params_sha256"])
