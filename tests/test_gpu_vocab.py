"""GPU tier: CTC vocabularies other than the 32 letters (1 <= vocab_size <= 1024), through the C ABI.

Goldens come from the reference's own code (tests/golden/make_golden_vocab.py), never from the NumPy oracle:
oracle/suta_loss_np.py divides the MCC term by V, the reference by its class_num default 32, so the oracle is
valid at V = 32 only.

Tolerances:
  * loss gradient vs the fp64 golden: max(2e-6, 2 * ref_f32_relerr) * max|g| + 1e-9.  2e-6 is the bound of
    test_gpu_parity.test_loss_kernel_matches_reference_autograd; ref_f32_relerr is the error of the reference's own
    fp32 run against its fp64 run, recorded per case (torch fp32 is 2.9e-6 off at V = 392, T = 1).
  * loss: 1e-5 * max(1, |loss|); NaN must match NaN.
  * adapted logits / tensors / bf16 mode: tests/parity.py, as the 32-class tests.
"""
import ast
import os

import numpy as np
import pytest

from suta_amd import synth
from suta_amd.config import get_config
from suta_amd.engine import SutaEngine, SutaHParams
from suta_amd.weights import synth_weights
from tests.parity import BF16_LOGITS_RTOL, assert_bf16_close, assert_params_close, logits_tol

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_ENGINES = {}


def engine(preset, V, max_batch=3, precision="fp32"):
    key = (preset, V, max_batch)
    if key not in _ENGINES:
        cfg = get_config(preset)
        cfg["vocab_size"] = V
        _ENGINES[key] = (SutaEngine(cfg, synth_weights(cfg), max_batch=max_batch), cfg)
    _ENGINES[key][0].set_precision(precision)
    return _ENGINES[key]


def _load(name):
    return np.load(os.path.join(G, name), allow_pickle=False)


def _hp(row):
    temp, em, rw, nb, div = row
    return SutaHParams(temp=float(temp), em_coef=float(em), reweight=bool(rw), non_blank=bool(nb), div_coef=float(div))


def _check_loss_case(eng, z, case, floor=2e-6):
    ref = z[f"{case}/grad_f64"]
    d, loss = eng.loss_grad(z[f"{case}/logits"], _hp(z[f"{case}/hp"]))
    rel = max(floor, 2.0 * float(z[f"{case}/ref_f32_relerr"])) if f"{case}/ref_f32_relerr" in z.files else floor
    gmax = float(np.abs(ref).max())
    err = float(np.abs(d[0].astype(np.float64) - ref).max())
    print(f"{case}: max|d| / max|g| = {err / gmax:.3g} (bound {rel:.3g}), loss {loss[0]!r}")
    assert err <= rel * gmax + 1e-9, (str(case), err / gmax, rel)
    rl = float(z[f"{case}/loss_f64"])
    if np.isnan(rl):
        assert np.isnan(loss[0]), case
    else:
        assert abs(loss[0] - rl) <= 1e-5 * max(1.0, abs(rl)), (case, loss[0], rl)


@pytest.mark.parametrize("fname", ["g10_vocab_loss_v33.npz", "g10_vocab_loss_v64.npz", "g10_vocab_loss_v65.npz",
                                   "g10_vocab_loss_v96.npz", "g10_vocab_loss_v96_cases.npz",
                                   "g10_vocab_loss_v392.npz", "g10_vocab_loss_v1024.npz"])
def test_loss_matches_reference_autograd(fname):
    """V = 33 and 64 run the one-block kernel (whose MCC divisor is the reference's 32, not V), V >= 65 the
    any-vocabulary path."""
    z = _load(fname)
    V = int(z[f"{z['cases'][0]}/logits"].shape[1])
    eng, _ = engine("tiny-group", V)
    for case in z["cases"]:
        _check_loss_case(eng, z, case)


@pytest.mark.parametrize("fname", ["g1_loss_grad.npz", "g10_vocab_loss_v33.npz", "g10_vocab_loss_v64.npz"])
def test_forced_wide_path_matches_reference_autograd(fname, monkeypatch):
    """SUTA_LOSS_WIDE=1 sends V <= 64 through the any-vocabulary kernels: the existing 32-class goldens at their own
    2e-6 bound, and the two other sizes both paths accept."""
    monkeypatch.setenv("SUTA_LOSS_WIDE", "1")
    z = _load(fname)
    V = int(z[f"{z['cases'][0]}/logits"].shape[1])
    eng, _ = engine("tiny-group", V)
    for case in z["cases"]:
        _check_loss_case(eng, z, case)


def test_loss_is_bitwise_repeatable_and_batched():
    """The same call twice gives the same bits, and a batch of utterances equals the utterances alone."""
    z = _load("g10_vocab_loss_v392.npz")
    eng, _ = engine("tiny-layer", 392)
    L = z["canon_V392_T70/logits"]
    hp = _hp(z["canon_V392_T70/hp"])
    batch = np.stack([L, L[::-1].copy(), np.roll(L, 3, axis=1)])
    d1, l1 = eng.loss_grad(batch, hp)
    d2, l2 = eng.loss_grad(batch, hp)
    assert np.array_equal(d1, d2) and np.array_equal(l1, l2)
    for b in range(3):
        ds, ls = eng.loss_grad(batch[b], hp)
        assert np.array_equal(ds[0], d1[b]) and ls[0] == l1[b], b


MODEL_CASES = [("group_v41", "tiny-group", 41), ("layer_v392", "tiny-layer", 392)]


@pytest.mark.parametrize("precision", ["fp32", "fp32-split-bf16"])
@pytest.mark.parametrize("variant,preset,V", MODEL_CASES)
def test_tiny_suta_matches_reference(variant, preset, V, precision):
    eng, cfg = engine(preset, V, precision=precision)
    for n in (8000, 12345):
        z = _load(f"g11_vocab_tiny_{variant}_N{n}.npz")
        h = ast.literal_eval(str(z["hp_json"]))
        steps = int(z["steps"])
        hp = SutaHParams(lr=h["lr"], temp=h["temp"], em_coef=h["em"], reweight=h["rw"], non_blank=h["nb"],
                         div_coef=h["div"], train_feature=h["train_feature"], bias_only=h["bias_only"])
        logits, ids, T = eng.adapt(z["x"], steps, hp, record=list(range(steps + 1)))
        ref = z["logits"]
        for i in range(steps + 1):
            np.testing.assert_allclose(logits[i][0], ref[i], rtol=0, atol=logits_tol(h["lr"]),
                                       err_msg=f"{variant} N{n} step {i}")
            np.testing.assert_array_equal(ids[i][0], logits[i][0].argmax(-1))
        for key in z.files:
            if key.startswith("final/"):
                name = key[len("final/"):]
                assert_params_close(eng.get_param(0, name), z[key], h["lr"], steps, name=name)


@pytest.mark.parametrize("variant,preset,V", MODEL_CASES)
def test_bf16_tiny_tracks_reference(variant, preset, V):
    """bf16 GEMM mode against the fp32 golden.  V = 392 is the issue's case (lm_head planes: K = V a multiple of 8);
    V = 41 is the odd size, where the lm_head input gradient (K = V, lda = V) must leave the bf16-plane kernels."""
    eng, cfg = engine(preset, V, precision="bf16")
    z = _load(f"g11_vocab_tiny_{variant}_N12345.npz")
    h = ast.literal_eval(str(z["hp_json"]))
    steps = int(z["steps"])
    logits, ids, T = eng.adapt(z["x"], steps, SutaHParams(lr=h["lr"]), record=list(range(steps + 1)))
    for i in range(steps + 1):
        assert_bf16_close(logits[i][0], z["logits"][i], 0.9, f"{variant} step {i}", rtol=BF16_LOGITS_RTOL)
        np.testing.assert_array_equal(ids[i][0], logits[i][0].argmax(-1))


def test_ragged_batch_equals_single_runs_v392():
    eng, cfg = engine("tiny-layer", 392)
    waves = [synth.wave(n, 140 + i) for i, n in enumerate((12345, 8000, 10007))]
    hp = SutaHParams(lr=5e-4)
    steps, record = 4, [0, 1, 4]
    lv, iv, tv = eng.adapt_varlen(waves, steps, hp, record=record)
    names = eng.trainable_names()
    finals = [{n: eng.get_param(b, n) for n in names} for b in range(len(waves))]
    for b, w in enumerate(waves):
        l1, i1, t1 = eng.adapt(w, steps, hp, record=record)
        assert tv[b] == t1
        for r in record:
            np.testing.assert_allclose(lv[r][b], l1[r][0], rtol=0, atol=logits_tol(hp.lr), err_msg=f"utt {b} step {r}")
            assert np.mean(iv[r][b] == i1[r][0]) > 0.99
        for n in names:
            assert_params_close(finals[b][n], eng.get_param(0, n), hp.lr, steps, name=f"utt {b} {n}")


def test_graph_replay_equals_eager_v392():
    eng, cfg = engine("tiny-layer", 392)
    x = synth.batch(11000, 2, start=150)
    hp = SutaHParams(lr=5e-4)
    eng.set_graphs(False)
    a, ia, _ = eng.adapt(x, 3, hp, record=[1, 3])
    assert eng.graph_stats()["last"] == "eager"
    eng.set_graphs(True)
    g0 = eng.graph_stats()
    b, ib, _ = eng.adapt(x, 3, hp, record=[1, 3])
    g1 = eng.graph_stats()
    c, ic, _ = eng.adapt(x, 3, hp, record=[1, 3])
    g2 = eng.graph_stats()
    assert g1["last"] == "captured" and g1["captures"] == g0["captures"] + 1
    assert g2["last"] == "replayed" and g2["captures"] == g1["captures"] and g2["launches"] == g1["launches"] + 1
    for r in (1, 3):
        assert np.array_equal(a[r], b[r]) and np.array_equal(a[r], c[r]), r
        assert np.array_equal(ia[r], ib[r]) and np.array_equal(ia[r], ic[r]), r


def test_vocab_cap_and_sdpl_refusal():
    cfg = get_config("tiny-group")
    cfg["vocab_size"] = 1025
    with pytest.raises(RuntimeError, match="1024"):
        SutaEngine(cfg, synth_weights(cfg), max_batch=1)
    eng, _ = engine("tiny-group", 41)
    L = np.zeros((5, 41), np.float32)
    with pytest.raises(RuntimeError, match="SDPL"):
        eng.loss_grad(L, SutaHParams(pl_coef=1.0))
