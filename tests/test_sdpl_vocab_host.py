"""Host side of the SDPL objective on any vocabulary (CPU): the pseudo-label table and the Python restatement of
the reference's target rule (main_SDPL.py:194-203 on Wav2Vec2CTCTokenizer.batch_decode), against the target ids the
reference itself built (tests/golden/make_golden_sdpl_vocab.py) and against the oracle's 32-letter rule."""
import glob
import json
import os

import numpy as np
import pytest

from oracle import w2v2_cpu as W
from suta_amd import decode as D
from suta_amd import main as M
from suta_amd.config import get_config

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_vocab(V):
    with open(os.path.join(G, f"g13_sdpl_vocab{V}.json"), encoding="utf-8") as f:
        raw = json.load(f)
    return D.CTCVocab(sorted(raw, key=raw.get))


def test_fixture_vocabularies_hold_what_the_cases_need():
    v = fixture_vocab(96)
    tab = D.pseudo_label_table(v)
    assert v.pad_id == 0 and v.tokens.index("|") not in (0, 4) and tab.space_id == v.tokens.index("|")
    multi = [i for i, t in enumerate(v.tokens) if len(t) > 1 and not t.startswith("<")]
    assert sum(tab.kinds[i] == D.KIND_NORMAL for i in multi) >= 8     # ch, sch, th, ...
    assert sum(tab.kinds[i] == D.KIND_FAIL for i in multi) >= 3       # a character that is no token
    for s in ("<s>", "</s>", "<unk>"):
        assert tab.kinds[v.tokens.index(s)] == D.KIND_FAIL
    i = v.tokens.index("sch")
    assert tab.ids[tab.offsets[i]:tab.offsets[i + 1]] == [v.tokens.index(c) for c in "sch"]
    assert tab.kinds[0] == D.KIND_DROP and tab.notice is None
    for V in (392, 1024):
        assert len(fixture_vocab(V)) == V


def test_target_equals_the_reference_built_target_of_every_golden_case():
    n = 0
    for fn in sorted(glob.glob(os.path.join(G, "g13_sdpl_loss_v*.npz"))):
        z = np.load(fn, allow_pickle=False)
        tab = D.pseudo_label_table(fixture_vocab(int(z["vocab_size"])))
        for case in z["cases"]:
            ids = z[f"{case}/logits"].argmax(-1)
            assert D.pseudo_label_target(ids, tab) == z[f"{case}/target"].tolist(), (fn, case)
            n += 1
    for fn in sorted(glob.glob(os.path.join(G, "g14_sdpl_vocab_tiny_*.npz"))):
        z = np.load(fn, allow_pickle=False)
        tab = D.pseudo_label_table(fixture_vocab(int(z["vocab_size"])))
        assert z["f64_same_target"].all()   # the reference's fp64 run adapts toward the same labels
        for i in range(int(z["steps"])):
            assert D.pseudo_label_target(z["logits"][i].argmax(-1), tab) == z[f"target{i}"].tolist(), (fn, i)
            n += 1
    assert n >= 20 + 20


def test_target_equals_the_oracle_32_letter_rule_on_random_rows():
    rng = np.random.default_rng(5)
    tab = D.pseudo_label_table(D.CTCVocab(D.VOCAB))
    for k in range(400):
        T = int(rng.integers(0, 40))
        p = rng.uniform(0.1, 0.9)
        ids = [int(rng.choice([0, 4])) if rng.uniform() < p else int(rng.integers(0, 32)) for _ in range(T)]
        if k % 3:   # most rows without the special tokens, so that most rows compare targets, not errors
            ids = [i if i not in (1, 2, 3) else 5 for i in ids]
        try:
            want = W.pseudo_label_target(ids)
        except KeyError:
            with pytest.raises(KeyError):
                D.pseudo_label_target(ids, tab)
            continue
        assert D.pseudo_label_target(ids, tab) == want == D.pseudo_label_target(ids)
    # the built-in table is the engine's default rule: pad, three failures, the delimiter, every other id itself
    assert tab.kinds == [D.KIND_DROP] + [D.KIND_FAIL] * 3 + [D.KIND_SPACE] + [D.KIND_NORMAL] * 27
    assert tab.ids == list(range(5, 32)) and tab.space_id == 4 and tab.offsets == [0] * 6 + list(range(1, 28))


def test_expansion_strip_and_inner_space():
    v = D.CTCVocab(["<pad>", "_", "c", "h", "ch", "|", "xy"], word_delimiter_token="_")
    # "_" is the delimiter, the literal bar an ordinary token: an inner space maps to vocab['|'] = 5
    assert D.pseudo_label_target([1, 1, 2, 4, 0, 1, 0, 1, 3, 1], v) == [2, 2, 3, 5, 5, 3]
    with pytest.raises(KeyError):
        D.pseudo_label_target([2, 6], v)                       # 'x' is no token
    nobar = D.CTCVocab(["<pad>", "_", "c"], word_delimiter_token="_")
    assert D.pseudo_label_target([1, 2, 1], nobar) == [2]     # the spaces at both ends vanish
    with pytest.raises(KeyError):
        D.pseudo_label_target([2, 1, 2], nobar)                # an inner space needs vocab['|']


def test_table_refuses_what_it_cannot_express():
    with pytest.raises(ValueError, match="whitespace"):
        D.pseudo_label_table(D.CTCVocab(["<pad>", "|", "a", " x"]))
    with pytest.raises(ValueError, match="id 0"):
        D.pseudo_label_table(D.CTCVocab(["a", "|", "ab", "b", "<pad>"]))   # "ab" expands to id 0
    note = D.pseudo_label_table(D.CTCVocab(["<unk>", "|", "b", "<pad>"])).notice
    assert note and "id 3" in note and "id 0" in note                     # pad is not the CTC blank
    assert "not in vocab.json" in D.pseudo_label_table(D.CTCVocab(["<unk>", "|", "b"])).notice


def _run_cli(tmp_path, vocab, capsys):
    d = tmp_path / "ckpt"
    d.mkdir()
    (d / "vocab.json").write_text(json.dumps(vocab, ensure_ascii=False), encoding="utf-8")
    argv = f"--asr {d} --dataset_name chime --dataset_dir {tmp_path}/none --log_dir {tmp_path}/exps --episodic".split()
    with pytest.raises((SystemExit, Exception)) as ei:   # there is no dataset and no model behind the vocabulary
        M.main(argv, sdpl=True)
    return capsys.readouterr().out, ei.value


def test_sdpl_cli_prints_the_directory_vocabulary(tmp_path, capsys):
    with open(os.path.join(G, "g13_sdpl_vocab96.json"), encoding="utf-8") as f:
        vocab = json.load(f)
    out, _ = _run_cli(tmp_path, vocab, capsys)
    assert out.splitlines()[0] == str(vocab)                  # main_SDPL.py:269-271 prints vocab.json


def test_sdpl_cli_exits_on_an_inexpressible_vocabulary(tmp_path, capsys):
    out, err = _run_cli(tmp_path, {"<pad>": 0, "|": 1, "a": 2, "b c": 3}, capsys)
    assert isinstance(err, SystemExit) and "whitespace" in str(err) and "SDPL" in str(err)


def test_budget_estimate_counts_the_sdpl_plane():
    cfg = dict(get_config("wav2vec2-base"), vocab_size=1024)
    assert M.workspace_bytes_per_audio_s(cfg, sdpl=True) - M.workspace_bytes_per_audio_s(cfg) == 50 * 4 * 1024
