"""GPU tier: the XLS-R geometries -- hidden sizes up to 2048, positional-conv groups of width 80 / 120, and head dims
80 / 120 on the flash attention kernels of csrc/attn_wide.hip (forward: ctx + LSE; backward: P recomputed, dQ / dK /
dV; no T x T matrix stored).

Tolerances are the project's own for each comparison:
  * full-width models against the CPU oracle: atol 5e-5 on logits (test_base_suta_matches_reference)
  * tiny models against the CPU oracle: tests/parity.logits_tol(lr)
  * flash against the P-storing GEMM path: atol 2e-5 on logits (test_fused_attention_equals_unfused), adapted tensors
    by tests/parity.assert_params_close
  * bf16 mode against exact fp32: tests/parity.assert_bf16_close
"""
import re

import numpy as np
import pytest
import torch

from suta_amd import synth
from suta_amd.config import get_config, num_frames
from suta_amd.engine import SutaEngine, SutaHParams
from suta_amd.weights import synth_weights
from tests.parity import assert_bf16_close, assert_params_close, logits_tol

pytestmark = pytest.mark.gpu

TINY = ["tiny-hd80", "tiny-hd120"]
_CACHE = {}


def wide_cfg(hidden):
    """One XLS-R-shaped layer at full width: 16 heads (head dim hidden / 16), 16 positional-conv groups."""
    cfg = get_config("wav2vec2-xls-r-1b")
    cfg.update(hidden_size=hidden, num_attention_heads=16, num_conv_pos_embedding_groups=16, num_hidden_layers=1,
               intermediate_size=256, conv_dim=[32] * 7)
    return cfg


def model(key):
    """(cfg, weights) of a tiny preset or of wide_cfg(hidden) for key 'h<hidden>'; built once."""
    if ("model", key) not in _CACHE:
        cfg = wide_cfg(int(key[1:])) if key.startswith("h") else get_config(key)
        _CACHE[("model", key)] = (cfg, synth_weights(cfg))
    return _CACHE[("model", key)]


def engine(key, fused=True, monkeypatch=None):
    """The shared engine of a model (max_batch 2); fused=False: built with SUTA_ATTN_FUSED=0 (the P-storing path)."""
    if ("engine", key, fused) not in _CACHE:
        cfg, sd = model(key)
        if not fused:
            monkeypatch.setenv("SUTA_ATTN_FUSED", "0")
        _CACHE[("engine", key, fused)] = SutaEngine(cfg, sd, max_batch=2, max_samples=128000)
        if not fused:
            monkeypatch.delenv("SUTA_ATTN_FUSED")
    eng = _CACHE[("engine", key, fused)]
    eng.set_precision("fp32")
    return eng


def oracle(key, x, steps, record):
    from oracle import w2v2_cpu as W
    cfg, sd = model(key)
    ref, _ = W.run_suta({k: torch.from_numpy(v) for k, v in sd.items()}, cfg, torch.from_numpy(x)[None], steps,
                        record=record)
    return {r: ref[r][0].numpy() for r in record}


@pytest.mark.parametrize("hidden", [1280, 1920])
def test_wide_hidden_matches_oracle(hidden):
    """hidden 1280 / 1920 (head dims 80 / 120, group widths 80 / 120, LayerNorm over more than 1024 columns): the
    engine is created and two SUTA steps at N = 32 000 (T = 99) track the CPU oracle within the full-width tolerance."""
    eng = engine(f"h{hidden}")
    x = synth.wave(32000, 41)
    logits, ids, T = eng.adapt(x, 2, SutaHParams(), record=[0, 1, 2])
    assert T == 99
    ref = oracle(f"h{hidden}", x, 2, [0, 1, 2])
    for r in (0, 1, 2):
        err = float(np.abs(logits[r][0] - ref[r]).max())
        print(f"hidden {hidden} step {r}: max |engine - oracle| = {err:.3g}")
        np.testing.assert_allclose(logits[r][0], ref[r], rtol=0, atol=5e-5, err_msg=f"hidden {hidden} step {r}")


@pytest.mark.parametrize("preset", TINY)
def test_flash_is_what_runs(preset, monkeypatch):
    """Head dims 80 / 120 take the fused attention kernels: timing family 7 counts their launches, the GEMM census
    holds no attention GEMM (while the engine built with SUTA_ATTN_FUSED=0 shows them), and the
    workspace is smaller than the P-storing engine's by the T x T matrices less the flash scratch."""
    cfg, _ = model(preset)
    eng = engine(preset)
    n = 128000
    T, d = num_frames(cfg, n), cfg["hidden_size"] // cfg["num_attention_heads"]
    x = np.stack([synth.wave(n, 51), synth.wave(n, 52)])
    def census_of(e):
        """(attention-family launches, attention GEMM shapes) of one eager SUTA step: every attention product has
        M = T with (N, K) = (T, dh) (S, dP) or (dh, T) (ctx, dQ, dK, dV)"""
        e.set_graphs(False)
        e.set_timing(True)
        e.set_census(True)
        e.adapt(x, 1, SutaHParams(), record=[1])
        shapes = e.get_gemm_shape_times()
        launches = e.get_timing_ex()["attention"][1]
        e.set_census(False)
        e.set_timing(False)
        e.set_graphs(True)
        assert shapes, "census + timing give the per-shape table"
        mnk = {k: tuple(int(re.search(rf"\b{c}=(\d+)", k).group(1)) for c in "MNK") for k in shapes}
        return launches, [k for k, v in mnk.items() if v in ((T, T, d), (T, d, T))]

    L = cfg["num_hidden_layers"]
    launches, attn_gemms = census_of(eng)
    # 2 forwards (grad + re-inference) and 1 backward (kernel + dQ reduction) per layer and step, + the vanilla forward
    assert launches >= 3 * L, launches
    assert not attn_gemms, attn_gemms
    ws = eng.workspace_bytes()
    ref = engine(preset, fused=False, monkeypatch=monkeypatch)
    launches, attn_gemms = census_of(ref)   # the P-storing path: the check above can see what it excludes
    assert launches == 0 and attn_gemms, (launches, attn_gemms)
    B, NH, Tp, ng = 2, cfg["num_attention_heads"], -(-T // 4) * 4, -(-T // 32)
    p_bytes = 4 * (L + 1) * B * NH * T * Tp                        # P per layer + dP
    dq_bytes = 4 * -(-ng // 4) * B * NH * ng * 32 * 128            # dQ partials per key block of 128 (padded width <= 128)
    lse_bytes = 4 * L * B * NH * T
    assert ref.workspace_bytes() - ws >= p_bytes - dq_bytes - lse_bytes - 4096 * (L + 2), (ref.workspace_bytes(), ws)
    assert ws < ref.workspace_bytes()


@pytest.mark.parametrize("n", [400, 10960, 32000, 128000])
@pytest.mark.parametrize("preset", TINY)
def test_flash_equals_p_storing_path(preset, n, monkeypatch):
    """The head-dim 80 / 120 flash kernels against the S-GEMM / softmax / PV-GEMM path that stores P: 3 SUTA steps at
    T = 1, T = 34 (a second, partial 32-row tile), T = 99 and T = 399 (more than one key block in the backward), and a
    ragged pair (n, 3n/5; not at n = 400, where 240 samples are shorter than the conv stack's receptive field)."""
    eng = engine(preset)
    ref_eng = engine(preset, fused=False, monkeypatch=monkeypatch)
    hp = SutaHParams()
    x = synth.wave(n, 21)
    a, _, _ = ref_eng.adapt(x, 3, hp, record=[0, 3])
    pa = {name: ref_eng.get_param(0, name) for name in ref_eng.trainable_names()}
    b, _, _ = eng.adapt(x, 3, hp, record=[0, 3])
    for r in (0, 3):
        print(f"{preset} n={n} step {r}: max |flash - unfused| = {float(np.abs(b[r] - a[r]).max()):.3g}")
        np.testing.assert_allclose(b[r], a[r], rtol=0, atol=2e-5, err_msg=f"step {r}")
    for name, v in pa.items():
        assert_params_close(eng.get_param(0, name), v, hp.lr, 3, name=name)
    if n * 3 // 5 >= 400:
        waves = [synth.wave(n, 22), synth.wave(n * 3 // 5, 23)]
        a, _, _ = ref_eng.adapt_varlen(waves, 2, hp, record=[2])
        b, _, _ = eng.adapt_varlen(waves, 2, hp, record=[2])
        for u in range(2):
            np.testing.assert_allclose(b[2][u], a[2][u], rtol=0, atol=2e-5, err_msg=f"ragged utterance {u}")


@pytest.mark.parametrize("preset", TINY)
def test_tiny_head_dims_match_oracle(preset):
    eng = engine(preset)
    hp = SutaHParams()
    x = synth.wave(32000, 31)
    logits, ids, T = eng.adapt(x, 2, hp, record=[0, 1, 2])
    ref = oracle(preset, x, 2, [0, 1, 2])
    for r in (0, 1, 2):
        np.testing.assert_allclose(logits[r][0], ref[r], rtol=0, atol=logits_tol(hp.lr), err_msg=f"step {r}")
        np.testing.assert_array_equal(ids[r][0], logits[r][0].argmax(-1))


@pytest.mark.parametrize("key", TINY + ["h1280"])
def test_bf16_mode_tracks_fp32(key):
    """bf16 GEMM mode (the flash kernels' operands rounded to bf16, the bf16 planes of ctx and dQKV written for the
    plane GEMMs around attention; the new head dims read fp32 rows) against the same engine in exact fp32."""
    eng = engine(key)
    x = synth.wave(32000, 61)
    ref, _, _ = eng.adapt(x, 3, SutaHParams(), record=[0, 3])
    eng.set_precision("bf16")
    try:
        got, ids, _ = eng.adapt(x, 3, SutaHParams(), record=[0, 3])
    finally:
        eng.set_precision("fp32")
    for r in (0, 3):
        assert np.isfinite(got[r]).all()
        assert_bf16_close(got[r][0], ref[r][0], 0.9, f"{key} step {r}")
        np.testing.assert_array_equal(ids[r][0], got[r][0].argmax(-1))


def test_deterministic_and_graph_replay_equals_eager():
    """tiny-hd80: two identical adapt calls are bitwise equal (fixed summation order, no float atomics), and the
    replayed hipGraph of the loop gives the eager call's ids and adapted tensors bitwise."""
    cfg, sd = model("tiny-hd80")
    eng = SutaEngine(cfg, sd, max_batch=2, max_samples=128000)
    names = eng.trainable_names()
    x = np.stack([synth.wave(128000, 71), synth.wave(128000, 72)])
    hp, rec = SutaHParams(), [0, 2]
    eng.adapt(x, 2, hp, record=rec, want_logits=False)             # first call of the key: eager
    assert eng.graph_stats()["last"] == "eager"
    eng.adapt(x, 2, hp, record=rec, want_logits=False)             # captured, then launched
    assert eng.graph_stats()["last"] == "captured"
    _, ids_r, _ = eng.adapt(x, 2, hp, record=rec, want_logits=False)
    assert eng.graph_stats()["last"] == "replayed"
    par_r = {b: {n: eng.get_param(b, n) for n in names} for b in range(2)}
    l1, ids1, _ = eng.adapt(x, 2, hp, record=rec)                  # logits wanted: a new key, eager
    assert eng.graph_stats()["last"] == "eager"
    par_1 = {b: {n: eng.get_param(b, n) for n in names} for b in range(2)}
    eng.set_graphs(False)
    l2, ids2, _ = eng.adapt(x, 2, hp, record=rec)
    for r in rec:
        assert np.array_equal(l1[r], l2[r]), f"rerun differs at step {r}"
        assert np.array_equal(ids_r[r], ids1[r]), f"replayed ids != eager ids at step {r}"
    for b in range(2):
        for n in names:
            assert np.array_equal(par_1[b][n], eng.get_param(b, n)), f"rerun differs: slot {b} {n}"
            assert np.array_equal(par_r[b][n], par_1[b][n]), f"replayed != eager: slot {b} {n}"
    eng.close()


def test_48_layers_create_and_adapt():
    """The depth of XLS-R 1B / 2B at tiny width: the per-layer tables and the optimizer's run table hold 48 layers."""
    cfg = get_config("tiny-hd80")
    cfg["num_hidden_layers"] = 48
    eng = SutaEngine(cfg, synth_weights(cfg), max_batch=1, max_samples=32000)
    logits, ids, T = eng.adapt(synth.wave(16000, 81), 1, SutaHParams(), record=[0, 1])
    assert T == 49
    assert np.isfinite(logits[0]).all() and np.isfinite(logits[1]).all()
    for name in eng.trainable_names():
        assert np.isfinite(eng.get_param(0, name)).all(), name
    eng.close()
