"""GPU tier: the SDPL pseudo-label objective (main_SDPL.py:143-209) on any CTC vocabulary up to 1024 classes.

Goldens come from the reference's own main_SDPL.forward_and_adapt with the fixture vocabulary as its vocab.json and
tokenizer (tests/golden/make_golden_sdpl_vocab.py).  Tolerances are those of tests/test_gpu_sdpl.py: the
loss-and-grad kernels within max(4 x the reference's own fp32-vs-fp64 deviation, 5e-6 * max|g|) and the loss within
2e-5 * max(1, |loss|); adapted logits within tests/parity.sdpl_logits_tol, greedy ids agreeing on >= 90 % of
frames, adapted tensors within twice the Adam step budget.
"""
import json
import os

import numpy as np
import pytest

from suta_amd import decode as D
from suta_amd import synth
from suta_amd.config import get_config
from suta_amd.engine import SutaEngine, SutaHParams
from suta_amd.weights import synth_weights
from tests.parity import assert_params_close, sdpl_logits_tol

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_ENG = {}


def fixture_vocab(V):
    with open(os.path.join(G, f"g13_sdpl_vocab{V}.json"), encoding="utf-8") as f:
        raw = json.load(f)
    return D.CTCVocab(sorted(raw, key=raw.get))


def sdpl_weights(cfg, fail_ids):
    sd = synth_weights(cfg, blank_bias=0.0)
    sd["lm_head.bias"][list(fail_ids)] -= 30.0  # as the fixtures: keep lookup-failure ids off the greedy path
    return sd


def engine(preset, V, max_batch=3):
    """An engine of V classes whose pseudo labels follow the fixture vocabulary of that size (V = 32: built in)."""
    key = (preset, V, max_batch)
    if key not in _ENG:
        cfg = get_config(preset)
        cfg["vocab_size"] = V
        if V == 32:
            eng = SutaEngine(cfg, sdpl_weights(cfg, (1, 2, 3)), max_batch=max_batch)
        else:
            tab = D.pseudo_label_table(fixture_vocab(V))
            fail = [i for i, k in enumerate(tab.kinds) if k == D.KIND_FAIL]
            eng = SutaEngine(cfg, sdpl_weights(cfg, fail), max_batch=max_batch)
            assert eng.set_pseudo_labels(tab) is None
        _ENG[key] = (eng, cfg)
    return _ENG[key]


def _hp(row):
    temp, em, rw, nb, pl = row
    return SutaHParams(temp=float(temp), em_coef=float(em), reweight=bool(rw), non_blank=bool(nb), pl_coef=float(pl))


def _check_case(eng, z, case):
    d, loss = eng.loss_grad(z[f"{case}/logits"], _hp(z[f"{case}/hp"]))
    ref = z[f"{case}/grad_f64"]
    own = np.abs(z[f"{case}/grad_f32"] - ref).max()
    tol = max(4 * own, 5e-6 * np.abs(ref).max())
    err = np.abs(d[0] - ref).max()
    rl = float(z[f"{case}/loss_f64"])
    print(f"{case}: max|d| {err:.3g} (bound {tol:.3g}, reference fp32 {own:.3g}), loss {loss[0]!r} vs {rl!r}")
    np.testing.assert_allclose(d[0], ref, rtol=0, atol=tol, err_msg=str(case))
    if np.isnan(rl):
        assert np.isnan(loss[0]), case
    else:
        assert abs(loss[0] - rl) <= 2e-5 * max(1.0, abs(rl)), (case, loss[0], rl)


@pytest.mark.parametrize("V", [33, 96, 392, 1024])
def test_wide_loss_kernels_match_reference(V):
    """Through suta_loss_grad.  The parent of this change answers SUTA_ERR_UNSUPPORTED at every V > 32."""
    eng, _ = engine("tiny-group", V)
    n = 0
    for suffix in ("", "_long"):
        z = np.load(os.path.join(G, f"g13_sdpl_loss_v{V}{suffix}.npz"), allow_pickle=False)
        for case in z["cases"]:
            _check_case(eng, z, case)
            n += 1
    assert n >= 4


def test_builtin_table_is_bitwise_and_wide_path_is_toleranced(monkeypatch):
    """At 32 classes: the table built from the built-in VOCAB is the engine's default rule, so the 32-letter kernels
    keep running and the output is BITWISE that of an engine with no table.  SUTA_SDPL_WIDE=1 sends the same logits
    through the any-vocabulary kernels, whose sums run in another order: they agree with the 32-letter kernels, and
    with the reference's fp64 gradient, to the TOLERANCE of test_gpu_sdpl.test_sdpl_loss_kernel_matches_reference."""
    eng, _ = engine("tiny-group", 32)
    z = np.load(os.path.join(G, "g6_sdpl_loss.npz"), allow_pickle=False)
    for case in z["cases"]:
        L, hp = z[f"{case}/logits"], _hp(z[f"{case}/hp"])
        eng.set_pseudo_labels(None)
        d0, l0 = eng.loss_grad(L, hp)
        eng.set_pseudo_labels(D.CTCVocab(D.VOCAB))
        d1, l1 = eng.loss_grad(L, hp)
        assert d0.tobytes() == d1.tobytes() and l0.tobytes() == l1.tobytes(), case
        monkeypatch.setenv("SUTA_SDPL_WIDE", "1")
        d2, l2 = eng.loss_grad(L, hp)
        monkeypatch.delenv("SUTA_SDPL_WIDE")
        ref = z[f"{case}/grad_f64"]
        own = np.abs(z[f"{case}/grad_f32"] - ref).max()
        tol = max(4 * own, 5e-6 * np.abs(ref).max())
        print(f"{case}: wide vs 32-letter {np.abs(d2 - d0).max():.3g}, wide vs fp64 {np.abs(d2[0] - ref).max():.3g}, "
              f"bound {tol:.3g}")
        np.testing.assert_allclose(d2, d0, rtol=0, atol=tol, err_msg=str(case))
        np.testing.assert_allclose(d2[0], ref, rtol=0, atol=tol, err_msg=str(case))
        rl = float(z[f"{case}/loss_f64"])
        if np.isnan(rl):
            assert np.isnan(l2[0]), case
        else:
            assert abs(l2[0] - rl) <= 2e-5 * max(1.0, abs(rl)), (case, l2[0], rl)
    eng.set_pseudo_labels(None)


@pytest.mark.parametrize("variant,preset,V", [("group_v41", "tiny-group", 41), ("layer_v392", "tiny-layer", 392)])
def test_tiny_adaptation_tracks_reference(variant, preset, V):
    eng, cfg = engine(preset, V)
    tab = D.pseudo_label_table(fixture_vocab(V))
    compared = recorded = 0
    for n in (8000, 5000):
        z = np.load(os.path.join(G, f"g14_sdpl_vocab_tiny_{variant}_N{n}.npz"), allow_pickle=False)
        lr, steps = float(z["lr"]), int(z["steps"])
        hp = SutaHParams(lr=lr, em_coef=1.0, reweight=False, non_blank=True, pl_coef=1.0)
        logits, ids, T = eng.adapt(z["x"], steps, hp, record=list(range(steps + 1)))
        ref = z["logits"]
        recorded += steps + 1

        def same(upto):  # both runs adapted toward the same pseudo labels at every step < upto
            return all(D.pseudo_label_target(logits[i][0].argmax(-1), tab) == z[f"target{i}"].tolist()
                       for i in range(upto))
        for i in range(steps + 1):
            if not same(i):
                break  # a greedy flip changed the CTC target: the runs adapt toward different labels
            np.testing.assert_allclose(logits[i][0], ref[i], rtol=0, atol=sdpl_logits_tol(lr, i),
                                       err_msg=f"{variant} N{n} step {i}")
            assert np.mean(ids[i][0] == ref[i].argmax(-1)) >= 0.9, (variant, n, i)
            compared += 1
        if same(steps):
            for key in z.files:
                if key.startswith("final/"):
                    name = key[len("final/"):]
                    assert_params_close(eng.get_param(0, name), z[key], lr, steps, max_frac=1.0, name=name, factor=2.0)
    print(f"{variant}: compared {compared} of {recorded} recorded steps")
    assert 3 * compared >= 2 * recorded  # the share test_gpu_sdpl.py demands (8 of 12)


def test_ragged_batch_equals_single_runs_v392():
    eng, cfg = engine("tiny-layer", 392)
    hp = SutaHParams(lr=1e-4, em_coef=1.0, reweight=False, pl_coef=1.0)
    waves = [synth.wave(n, 180 + i) for i, n in enumerate((9000, 12001, 8000))]
    lv, iv, tv = eng.adapt_varlen(waves, 3, hp, record=[0, 3])
    for b, w in enumerate(waves):
        l1, _, t1 = eng.adapt(w, 3, hp, record=[0, 3])
        assert tv[b] == t1
        np.testing.assert_allclose(lv[3][b], l1[3][0], rtol=0, atol=sdpl_logits_tol(1e-4, 3))


def _samples_for_frames(eng, T):
    n = 400
    while eng.num_frames(n) < T:
        n += 80
    assert eng.num_frames(n) == T
    return n


def test_error_paths_leave_the_engine_usable():
    cfg = get_config("tiny-group")
    cfg["vocab_size"] = 41
    toks = ["<pad>", "<s>", "</s>", "<unk>", "|", "a", "b", "c", "abc"] + list("defghijklmnopqrstuvwxyz012345678")
    vocab = D.CTCVocab(toks)
    hp = SutaHParams(pl_coef=1.0)
    # a bias that forces a lookup-failure token on every frame
    sd = synth_weights(cfg, blank_bias=0.0)
    sd["lm_head.bias"][3] += 50.0
    eng = SutaEngine(cfg, sd, max_batch=1)
    eng.set_pseudo_labels(vocab)
    with pytest.raises(RuntimeError, match="special token"):
        eng.adapt(synth.wave(8000, 1), 1, hp, record=[1])
    eng.close()
    # every frame decodes to "abc": one token, three labels, two frames
    sd = synth_weights(cfg, blank_bias=0.0)
    sd["lm_head.bias"][8] += 50.0
    eng = SutaEngine(cfg, sd, max_batch=1)
    eng.set_pseudo_labels(vocab)
    short = synth.wave(_samples_for_frames(eng, 2), 2)
    with pytest.raises(RuntimeError, match="pseudo label longer than the utterance allows"):
        eng.adapt(short, 1, hp, record=[1])
    with pytest.raises(RuntimeError, match="pseudo label longer than the utterance allows"):
        eng.loss_grad(eng.forward(short), hp)
    logits, ids, T = eng.adapt(synth.wave(8000, 2), 2, hp, record=[0, 2])   # 24 frames hold a b c
    assert T >= 3 and np.isfinite(logits[2]).all() and (ids[0][0] == 8).all()
    d, loss = eng.loss_grad(logits[0], hp)
    assert np.isfinite(d).all() and np.isfinite(loss).all()
    eng.close()


def test_malformed_table_is_an_argument_error():
    eng, _ = engine("tiny-group", 33)
    good = D.pseudo_label_table(fixture_vocab(33))
    z = np.load(os.path.join(G, "g13_sdpl_loss_v33.npz"), allow_pickle=False)
    case = z["cases"][1]
    before = eng.loss_grad(z[f"{case}/logits"], _hp(z[f"{case}/hp"]))[0]

    def bad(**kw):
        f = dict(offsets=list(good.offsets), ids=list(good.ids), kinds=list(good.kinds), space_id=good.space_id)
        f.update(kw)
        return D.PseudoLabelTable(f["offsets"], f["ids"], f["kinds"], f["space_id"])
    off = list(good.offsets)
    off[10], off[11] = off[11], off[10] - 1
    ids_hi, ids_zero, kinds = list(good.ids), list(good.ids), list(good.kinds)
    ids_hi[3], ids_zero[3], kinds[7] = 33, 0, 4
    for tab in (bad(offsets=off), bad(ids=ids_hi), bad(ids=ids_zero), bad(kinds=kinds), bad(space_id=33),
                bad(space_id=0)):
        with pytest.raises(RuntimeError, match="libsuta error 1: pseudo-label table"):
            eng.set_pseudo_labels(tab)
    after = eng.loss_grad(z[f"{case}/logits"], _hp(z[f"{case}/hp"]))[0]
    assert before.tobytes() == after.tobytes()   # a refused table leaves the one in place


def test_graph_replays_and_a_new_table_is_never_replayed():
    eng, cfg = engine("tiny-group", 96, max_batch=1)
    vocab = fixture_vocab(96)
    tab = D.pseudo_label_table(vocab)
    hp = SutaHParams(lr=1e-4, em_coef=1.0, reweight=False, pl_coef=1.0)
    x = synth.wave(8000, 190)
    a, _, _ = eng.adapt(x, 2, hp, record=[0, 2])
    b, _, _ = eng.adapt(x, 2, hp, record=[0, 2])
    g1 = eng.graph_stats()
    c, _, _ = eng.adapt(x, 2, hp, record=[0, 2])
    g2 = eng.graph_stats()
    assert g1["last"] == "captured" and g2["last"] == "replayed" and g2["captures"] == g1["captures"], (g1, g2)
    assert a[2].tobytes() == b[2].tobytes() == c[2].tobytes()
    # another table: the multi-character tokens become lookup failures, which this utterance's greedy path meets or
    # not -- either way the old capture must not run
    kinds = [D.KIND_FAIL if (k == D.KIND_NORMAL and tab.offsets[i + 1] - tab.offsets[i] > 1) else k
             for i, k in enumerate(tab.kinds)]
    offsets, ids = [0], []
    for i, k in enumerate(kinds):
        if k == D.KIND_NORMAL:
            ids += tab.ids[tab.offsets[i]:tab.offsets[i + 1]]
        offsets.append(len(ids))
    eng.set_pseudo_labels(D.PseudoLabelTable(offsets, ids, kinds, tab.space_id))
    try:
        eng.adapt(x, 2, hp, record=[0, 2])
    except RuntimeError as err:
        assert "special token" in str(err)
    g3 = eng.graph_stats()
    assert g3["last"] != "replayed" and g3["launches"] == g2["launches"], g3
    eng.set_pseudo_labels(tab)
    d, _, _ = eng.adapt(x, 2, hp, record=[0, 2])
    assert eng.graph_stats()["last"] == "eager" and d[2].tobytes() == a[2].tobytes()


def test_sdpl_driver_follows_the_checkpoint_vocabulary(tmp_path, capsys):
    """main_SDPL.py drop-in on a checkpoint directory with its own 41-token vocab.json: prints that vocabulary, sets
    the engine's table from it and adapts (the vanilla WER is counted over the same references at every step)."""
    from safetensors.numpy import save_file
    from suta_amd import main as M
    from tests import corpus_fixtures as CF
    CF.chime(tmp_path, n=2)
    cfg = get_config("tiny-group")
    cfg["vocab_size"] = 41
    with open(os.path.join(G, "g13_sdpl_vocab41.json"), encoding="utf-8") as f:
        vocab = json.load(f)
    sd = sdpl_weights(cfg, (1, 2, 3))
    sd["lm_head.bias"][[vocab["TH"], vocab["CH"]]] -= 30.0  # single-character labels only: every target fits
    ck = tmp_path / "ckpt"
    ck.mkdir()
    json.dump(cfg, open(ck / "config.json", "w"))
    json.dump(vocab, open(ck / "vocab.json", "w"))
    save_file(sd, str(ck / "model.safetensors"))
    args = (f"--asr {ck} --steps 3 --dataset_name chime --dataset_dir {tmp_path} --episodic "
            f"--log_dir {tmp_path}/exps --train_feature --pl_coef 1").split()
    counts = M.main(args, sdpl=True)
    out = capsys.readouterr().out
    assert out.splitlines()[0] == str(vocab) and "pl_coef = 1.0" in out
    assert counts["3"][1] == counts["0"][1] > 0


def test_above_32_classes_sdpl_waits_for_a_table():
    """The 32-letter rule names no vocabulary above 32 classes: with no table SDPL stays refused there (before any
    launch), a table lifts the refusal, and taking the table away brings it back."""
    cfg = get_config("tiny-group")
    cfg["vocab_size"] = 41
    eng = SutaEngine(cfg, sdpl_weights(cfg, (1, 2, 3)), max_batch=1)
    hp = SutaHParams(em_coef=1.0, reweight=False, non_blank=False, pl_coef=1.0)
    L = np.zeros((5, 41), np.float32)   # an all-blank greedy path: an empty pseudo label
    x = synth.wave(8000, 3)
    for call in (lambda: eng.loss_grad(L, hp), lambda: eng.adapt(x, 1, hp, record=[1]), lambda: eng.step(x, hp)):
        with pytest.raises(RuntimeError, match="libsuta error 3: SDPL objective at vocab_size > 32 needs"):
            call()
    eng.adapt(x, 1, SutaHParams(), record=[1])                   # SUTA alone never needed one
    eng.set_pseudo_labels(fixture_vocab(41))
    d, loss = eng.loss_grad(L, hp)
    assert np.isfinite(d).all() and np.isfinite(loss).all()
    eng.set_pseudo_labels(None)
    with pytest.raises(RuntimeError, match="SDPL"):
        eng.loss_grad(L, hp)
    eng.close()
