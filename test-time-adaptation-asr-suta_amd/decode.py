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


def load_vocab(path: str, target_lang=None) -> CTCVocab:
    """The vocabulary of a local HF checkpoint directory: vocab.json (token -> id) and, where present, the pad,
    word-delimiter and unk token names of tokenizer_config.json / special_tokens_map.json (HF defaults otherwise).
    A vocab.json nested per language ({"eng": {...}, ...}: MMS) gives `target_lang`'s table, else the one
    tokenizer_config.json names as `target_lang`; a flat vocab.json ignores the argument."""
    import json
    import os
    with open(os.path.join(path, "vocab.json"), encoding="utf-8") as f:
        raw = json.load(f)
    if raw and all(isinstance(v, dict) for v in raw.values()):
        lang = target_lang
        tc = os.path.join(path, "tokenizer_config.json")
        if lang is None and os.path.isfile(tc):
            with open(tc, encoding="utf-8") as f:
                lang = json.load(f).get("target_lang")
        if lang is None:
            raise ValueError(f"{path}/vocab.json holds one vocabulary per language ({', '.join(sorted(raw)[:5])}, ...): "
                             "pass --target_lang")
        if lang not in raw:
            raise KeyError(f"language '{lang}' is not in {path}/vocab.json ({', '.join(sorted(raw)[:8])}, ...)")
        raw = raw[lang]
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


# pseudo-label table kinds (csrc/ops.h SDPL_KIND_*)
KIND_NORMAL, KIND_DROP, KIND_SPACE, KIND_FAIL = 0, 1, 2, 3


class PseudoLabelTable:
    """How every class id of a vocabulary enters the SDPL pseudo-label target (main_SDPL.py:194-203):
    offsets (V + 1) and ids: id i expands to ids[offsets[i]:offsets[i + 1]]; kinds (V): KIND_NORMAL (its characters'
    ids), KIND_DROP (the pad token), KIND_SPACE (the word delimiter) or KIND_FAIL (a character of the token is no
    token: the reference's vocab lookup raises KeyError); space_id: what a space inside the transcript maps to
    (vocab['|'], the literal bar the reference hard-codes), -1 when vocab.json has no '|'; notice: a warning for the
    user, or None."""

    def __init__(self, offsets, ids, kinds, space_id, notice=None):
        self.offsets, self.ids, self.kinds, self.space_id, self.notice = offsets, ids, kinds, space_id, notice


def _as_vocab(vocab) -> CTCVocab:
    return vocab if isinstance(vocab, CTCVocab) else CTCVocab(list(vocab), pad_token=vocab[PAD_ID])


def pseudo_label_table(vocab) -> PseudoLabelTable:
    """The pseudo-label table of a CTCVocab (or a token list with pad = id 0, delimiter '|').

    The reference decodes the greedy ids with processor.batch_decode and maps every character of that string
    through vocab.json, a space as '|' (main_SDPL.py:197-202).  Per class id that is: the pad token gives nothing,
    the word delimiter a space (strip() removes those at both ends of the utterance), any other token the ids of
    its characters.  Raises ValueError for a vocabulary this cannot express exactly: a token other than the
    delimiter that contains whitespace (strip() and the ' ' -> '|' rule would then act inside tokens), an
    expansion that contains id 0 (nn.CTCLoss(blank=0) would read the label as blank), or two ids that decode to the
    same string and could be grouped by the tokenizer while the engine groups by id."""
    v = _as_vocab(vocab)
    toks = v.tokens
    index = {}
    for i, t in enumerate(toks):
        index.setdefault(t, i)
    offsets, ids, kinds = [0], [], []
    for i, t in enumerate(toks):
        kind = KIND_NORMAL
        if t == v.pad_token:
            kind = KIND_DROP
        elif t == v.word_delimiter_token:
            kind = KIND_SPACE
        else:
            if any(ch.isspace() for ch in t):
                raise ValueError(f"token {t!r} (id {i}) contains whitespace: the reference strips the decoded string "
                                 "and maps every space to '|' (main_SDPL.py:197-202), which a per-token table "
                                 "cannot express")
            exp = [index.get(ch, -1) for ch in t]
            if any(e < 0 for e in exp):
                kind = KIND_FAIL
            elif 0 in exp:
                raise ValueError(f"token {t!r} (id {i}) expands to id 0 ({toks[0]!r}), which nn.CTCLoss(blank=0) "
                                 "reads as the blank (main_SDPL.py:195)")
            else:
                ids.extend(exp)
        kinds.append(kind)
        offsets.append(len(ids))
    for i, t in enumerate(toks):
        if index[t] != i and not (kinds[i] == KIND_FAIL and kinds[index[t]] == KIND_FAIL):
            raise ValueError(f"ids {index[t]} and {i} both decode to {t!r}: the tokenizer groups repeats by string, "
                             "the engine by id")
    space_id = index.get(WORD_DELIM, -1)
    if space_id == 0:
        raise ValueError(f"'{WORD_DELIM}' is id 0: a space inside the transcript would become the CTC blank "
                         "(main_SDPL.py:195, 200-202)")
    notice = None
    if v.pad_id != PAD_ID:
        where = f"id {v.pad_id}" if v.pad_id is not None else "not in vocab.json"
        notice = (f"[suta_amd] pad token '{v.pad_token}' is {where}, but the pseudo-label CTC loss uses id {PAD_ID} "
                  f"({toks[PAD_ID]!r}) as its blank as the reference hard-codes it (main_SDPL.py:195)")
    return PseudoLabelTable(offsets, ids, kinds, space_id, notice)


def pseudo_label_target(ids: Sequence[int], vocab=VOCAB) -> List[int]:
    """The reference's pseudo-label target of a greedy id row for any vocabulary (main_SDPL.py:196-202 on
    Wav2Vec2CTCTokenizer.batch_decode): group repeats, drop pad, expand every token to its characters' ids,
    the delimiter to a space, strip the spaces at both ends, map the inner ones to vocab['|'].  KeyError where the
    reference's lookup fails."""
    tab = vocab if isinstance(vocab, PseudoLabelTable) else pseudo_label_table(vocab)
    out: List[int] = []   # -1 = a space
    prev = None
    for i in ids:
        i = int(i)
        if i == prev:
            continue
        prev = i
        k = tab.kinds[i]
        if k == KIND_DROP:
            continue
        if k == KIND_FAIL:
            raise KeyError(f"id {i}: a character of the token is not in the vocabulary (reference vocab lookup fails)")
        if k == KIND_SPACE:
            out.append(-1)
        else:
            out.extend(tab.ids[tab.offsets[i]:tab.offsets[i + 1]])
    while out and out[0] == -1:
        out.pop(0)
    while out and out[-1] == -1:
        out.pop()
    if -1 in out and tab.space_id < 0:
        raise KeyError(f"'{WORD_DELIM}' is not in the vocabulary (reference vocab lookup of a space fails)")
    return [tab.space_id if o == -1 else o for o in out]


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
