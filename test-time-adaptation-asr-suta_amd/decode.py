"""Greedy CTC decode and corpus WER (host side, reference row f1).

decode: Wav2Vec2CTCTokenizer.batch_decode of argmax ids as main.py:333-334 uses it
        (HF tokenization_wav2vec2.py:297-340, 411-450): group repeated tokens, drop the pad
        token, map the word delimiter to a space, join, strip.  The built-in table is the 32-letter
        vocabulary; load_vocab reads any local checkpoint's vocab.json and tokenizer files.
wer:    jiwer.wer(truth, hypothesis) (main.py:336, 408-434) restated: word-level Levenshtein
        after jiwer's default transform (collapse whitespace, strip, split on spaces), corpus
        WER = sum of (S + D + I) over pairs / sum of reference words.
"""
from __future__ import annotations

import re
from typing import List, Sequence, Tuple

import numpy as np

# facebook/wav2vec2-base-960h vocabulary (the reference ships the same table as vocab.json)
VOCAB = ["<pad>", "<s>", "</s>", "<unk>", "|", "E", "T", "A", "O", "N", "I", "H", "S", "R", "D", "L", "U", "M",
         "W", "C", "F", "G", "Y", "P", "B", "V", "K", "'", "X", "J", "Q", "Z"]
PAD_ID = 0
WORD_DELIM = "|"


class CTCVocab:
    """A checkpoint's CTC vocabulary: id -> token table and the pad / word-delimiter / unk token names."""

    def __init__(self, tokens: Sequence[str], pad_token: str = "<pad>", word_delimiter_token: str = WORD_DELIM,
                 unk_token: str = "<unk>"):
        self.tokens = list(tokens)
        self.pad_token, self.word_delimiter_token, self.unk_token = pad_token, word_delimiter_token, unk_token
        self.pad_id = self.tokens.index(pad_token) if pad_token in self.tokens else None

    def __len__(self):
        return len(self.tokens)


def _token_name(v, default):
    """tokenizer_config.json / special_tokens_map.json store a token as a string or as {"content": ...}."""
    if isinstance(v, dict):
        v = v.get("content")
    return v if isinstance(v, str) else default


def load_vocab(path: str) -> CTCVocab:
    """The vocabulary of a local HF checkpoint directory: vocab.json (token -> id) and, where present, the pad,
    word-delimiter and unk token names of tokenizer_config.json / special_tokens_map.json (HF defaults otherwise)."""
    import json
    import os
    with open(os.path.join(path, "vocab.json"), encoding="utf-8") as f:
        raw = json.load(f)
    n = max(raw.values()) + 1
    names = {"pad_token": "<pad>", "word_delimiter_token": WORD_DELIM, "unk_token": "<unk>"}
    for fn in ("special_tokens_map.json", "tokenizer_config.json"):   # the config wins, as in from_pretrained
        fp = os.path.join(path, fn)
        if os.path.isfile(fp):
            with open(fp, encoding="utf-8") as f:
                cfg = json.load(f)
            for k in names:
                if k in cfg:
                    names[k] = _token_name(cfg[k], names[k])
    tokens = [names["unk_token"]] * n   # an id vocab.json does not list decodes as unk
    for t, i in raw.items():
        tokens[i] = t
    return CTCVocab(tokens, **names)


def blank_notice(vocab: CTCVocab):
    """The reference hard-codes id 0 as the CTC blank in its non-blank mask (main.py:178-184) and the engine follows
    it; a checkpoint whose pad token has another id adapts with a mask on the wrong class.  None when id 0 is pad."""
    if vocab.pad_id == PAD_ID:
        return None
    where = f"id {vocab.pad_id}" if vocab.pad_id is not None else "not in vocab.json"
    return (f"[suta_amd] pad token '{vocab.pad_token}' is {where}, but the non-blank mask of the adaptation loss "
            f"tests id {PAD_ID} as the reference hard-codes it (main.py:178-184); decoding drops '{vocab.pad_token}'")


def ctc_decode(ids: Sequence[int], vocab=VOCAB) -> str:
    """group repeats -> drop pad -> delimiter to ' ' -> join -> strip (special tokens kept verbatim), as
    Wav2Vec2CTCTokenizer.batch_decode; tokens may be several characters long.  vocab: a token list (pad = id 0,
    delimiter '|') or a CTCVocab."""
    if isinstance(vocab, CTCVocab):
        table, pad, delim, unk = vocab.tokens, vocab.pad_token, vocab.word_delimiter_token, vocab.unk_token
    else:
        table, pad, delim, unk = vocab, vocab[PAD_ID], WORD_DELIM, "<unk>"
    out: List[str] = []
    prev = None
    for i in ids:
        i = int(i)
        tok = table[i] if 0 <= i < len(table) else unk
        if tok == prev:
            continue
        prev = tok
        if tok == pad:
            continue
        out.append(" " if tok == delim else tok)
    return "".join(out).strip()


def batch_decode(ids: np.ndarray, vocab=VOCAB) -> List[str]:
    ids = np.asarray(ids)
    if ids.ndim == 1:
        ids = ids[None]
    return [ctc_decode(r, vocab) for r in ids]


def _words(s: str) -> List[str]:
    """jiwer wer_default: RemoveMultipleSpaces, Strip, ReduceToListOfListOfWords."""
    s = re.sub(r"\s\s+", " ", s).strip()
    return [w for w in s.split(" ") if len(w) >= 1]


def edit_distance(ref: Sequence[str], hyp: Sequence[str]) -> int:
    """Levenshtein distance over word lists (S, D, I unit costs)."""
    n, m = len(ref), len(hyp)
    if n == 0:
        return m
    if m == 0:
        return n
    prev = list(range(m + 1))
    for i in range(1, n + 1):
        cur = [i] + [0] * m
        ri = ref[i - 1]
        for j in range(1, m + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ri != hyp[j - 1]))
        prev = cur
    return prev[m]


def wer_counts(truth: Sequence[str], hyp: Sequence[str]) -> Tuple[int, int]:
    """(total edits, total reference words) over sentence pairs."""
    if len(truth) != len(hyp):
        raise ValueError("truth and hypothesis lists differ in length")
    e = w = 0
    for t, h in zip(truth, hyp):
        tw = _words(t)
        if not tw:
            raise ValueError("one or more references are empty strings")  # jiwer raises too
        e += edit_distance(tw, _words(h))
        w += len(tw)
    return e, w


def wer(truth, hyp) -> float:
    if isinstance(truth, str):
        truth = [truth]
    if isinstance(hyp, str):
        hyp = [hyp]
    e, w = wer_counts(list(truth), list(hyp))
    return e / w
