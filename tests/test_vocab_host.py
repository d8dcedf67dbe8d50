"""Host side of the larger-vocabulary support (CPU): the checkpoint vocabulary loader, the CTC decode with
multi-character tokens against HF Wav2Vec2CTCTokenizer (tests/golden/make_golden_vocab.py g12), the pad-id notice."""
import json
import os
import shutil

import numpy as np

from suta_amd import decode as D
from suta_amd import main as M
from suta_amd.config import get_config

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _ckpt(tmp_path, tokenizer_config=None, special_tokens_map=None):
    shutil.copy(os.path.join(G, "g12_vocab96.json"), tmp_path / "vocab.json")
    if tokenizer_config is not None:
        (tmp_path / "tokenizer_config.json").write_text(json.dumps(tokenizer_config), encoding="utf-8")
    if special_tokens_map is not None:
        (tmp_path / "special_tokens_map.json").write_text(json.dumps(special_tokens_map), encoding="utf-8")
    return str(tmp_path)


def test_decode_matches_hf_tokenizer_on_96_token_vocab(tmp_path):
    vocab = D.load_vocab(_ckpt(tmp_path))
    assert len(vocab) == 96 and vocab.pad_id == 17
    assert any(len(t) > 1 and not t.startswith("<") for t in vocab.tokens)   # multi-character tokens
    with open(os.path.join(G, "g12_ctc_decode_vocab96.json"), encoding="utf-8") as f:
        cases = json.load(f)
    assert len(cases) >= 100
    for c in cases:
        assert D.ctc_decode(c["ids"], vocab) == c["text"], c
    got = D.batch_decode(np.array([cases[1]["ids"]]), vocab)
    assert got == [cases[1]["text"]]


def test_builtin_table_is_unchanged():
    with open(os.path.join(G, "g5_ctc_decode.json")) as f:
        cases = json.load(f)
    for c in cases[:50]:
        assert D.ctc_decode(c["ids"]) == c["text"]
        assert D.ctc_decode(c["ids"], D.VOCAB) == c["text"]


def test_vocab_loader_reads_token_names_from_tokenizer_files(tmp_path):
    with open(os.path.join(G, "g12_vocab96.json"), encoding="utf-8") as f:
        raw = json.load(f)
    order = sorted(raw, key=raw.get)
    pad, delim = order[3], order[9]   # two ordinary tokens take the roles
    vocab = D.load_vocab(_ckpt(tmp_path, tokenizer_config={"pad_token": {"content": pad}, "word_delimiter_token": delim},
                               special_tokens_map={"pad_token": "<pad>", "unk_token": "<unk>"}))
    assert vocab.pad_token == pad and vocab.pad_id == 3 and vocab.word_delimiter_token == delim
    assert vocab.unk_token == "<unk>"
    ids = [1, 1, 3, 1, 9, 9, 2, 3, 3, 17, 500]
    assert D.ctc_decode(ids, vocab) == order[1] + order[1] + " " + order[2] + "<pad>" + "<unk>"
    # a gap in vocab.json decodes as unk
    d2 = tmp_path / "gap"
    d2.mkdir()
    (d2 / "vocab.json").write_text(json.dumps({"<pad>": 0, "a": 1, "b": 3}))
    v2 = D.load_vocab(str(d2))
    assert v2.tokens == ["<pad>", "a", "<unk>", "b"] and D.ctc_decode([1, 0, 1, 2, 3], v2) == "aa<unk>b"


def test_pad_id_notice(tmp_path):
    vocab = D.load_vocab(_ckpt(tmp_path))
    note = D.blank_notice(vocab)
    assert note and "id 17" in note and "id 0" in note
    assert D.blank_notice(D.CTCVocab(D.VOCAB)) is None
    assert "not in vocab.json" in D.blank_notice(D.CTCVocab(["a", "b"]))


def test_budget_estimate_grows_with_vocabulary():
    base = get_config("wav2vec2-base")
    wide = dict(base, vocab_size=1024)
    assert M.workspace_bytes_per_audio_s(wide) - M.workspace_bytes_per_audio_s(base) == 50 * 4 * 2 * (1024 - 32)
