"""BERT WordPiece tokenizer through the C-ABI (vr_wordpiece_*, csrc/wordpiece.cpp): the tokenise
step of SentenceTransformer.encode (reference: src/voitta/services/embedding.py:40,68-73 -> [EXT]
HF tokenizers). Returns packed ids + offsets, the form vr_encode / vr_index_batch take."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

from ._lib import check, load_library


DEFAULT_SPECIALS = ("[CLS]", "[SEP]", "[UNK]")


def wordpiece_specials(spec: dict) -> tuple[str, str, str]:
    """(cls, sep, unk) token names of a WordPiece tokenizer.json: from its post_processor — a BertProcessing or
    RobertaProcessing ("cls" / "sep" pairs), or a TemplateProcessing whose single-sequence template is
    <special> $A <special> — and the model's unk_token. A tokenizer.json without a post_processor wraps nothing, and
    any other template is not what the native tokenizer produces: both raise ValueError (the caller then takes the
    tokenizers library)."""
    post = spec.get("post_processor") or {}
    kind = post.get("type")
    if kind in ("BertProcessing", "RobertaProcessing"):
        cls_tok, sep_tok = post["cls"][0], post["sep"][0]
        ids = {cls_tok: post["cls"][1], sep_tok: post["sep"][1]}
    elif kind == "TemplateProcessing":
        single = post.get("single") or []
        shape = [("SpecialToken" if "SpecialToken" in p else "Sequence") for p in single]
        if shape != ["SpecialToken", "Sequence", "SpecialToken"] or single[1]["Sequence"].get("id") != "A" \
                or any(p[k].get("type_id", 0) != 0 for p in single for k in p):
            raise ValueError("post_processor template is not '<cls> $A <sep>'")
        cls_tok, sep_tok = single[0]["SpecialToken"]["id"], single[2]["SpecialToken"]["id"]
        ids = {}
        for name in (cls_tok, sep_tok):
            entry = (post.get("special_tokens") or {}).get(name) or {}
            if len(entry.get("ids") or []) != 1:
                raise ValueError(f"post_processor special token {name!r} is not a single id")
            ids[name] = entry["ids"][0]
    else:
        raise ValueError(f"post_processor {kind!r} is not a <cls> $A <sep> wrapper")
    vocab = spec["model"]["vocab"]
    for name, i in ids.items():  # the native tokenizer finds the specials by name: the ids must be the vocabulary's
        if vocab.get(name) != i:
            raise ValueError(f"post_processor gives {name!r} id {i}, the vocabulary {vocab.get(name)}")
    return cls_tok, sep_tok, spec["model"].get("unk_token", "[UNK]")


class WordPieceTokenizer:
    def __init__(self, vocab: list[str], lowercase: bool = True, strip_accents: bool | None = None,
                 handle_chinese_chars: bool = True, clean_text: bool = True, max_length: int = 512,
                 specials: tuple[str, str, str] = DEFAULT_SPECIALS):
        """specials: the (cls, sep, unk) token names — a sequence is cls ... sep, an unknown word unk. Other names than
        the default ([CLS], [SEP], [UNK]; MPNet: <s>, </s>, [UNK]) go through vr_wordpiece_create_specials."""
        self._lib = load_library()
        self.vocab_size = len(vocab)
        self.max_length = int(max_length)
        self.specials = tuple(specials)
        raw = [t.encode("utf-8") for t in vocab]
        arr = (C.c_char_p * len(raw))(*raw)
        h = C.c_void_p()
        flags = (int(lowercase), -1 if strip_accents is None else int(strip_accents), int(handle_chinese_chars),
                 int(clean_text))
        if self.specials == DEFAULT_SPECIALS:
            check(self._lib.vr_wordpiece_create(arr, len(raw), *flags, C.byref(h)))
        else:
            check(self._lib.vr_wordpiece_create_specials(arr, len(raw), *flags, *(t.encode("utf-8") for t in self.specials),
                                                         C.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.vr_wordpiece_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def from_pretrained(cls, path: str, max_length: int = 512) -> "WordPieceTokenizer":
        """vocab.txt (+ tokenizer_config.json) or tokenizer.json of a BERT checkpoint directory."""
        lowercase, strip, chinese, clean = True, None, True, True
        specials = DEFAULT_SPECIALS
        cfg_path = os.path.join(path, "tokenizer_config.json")
        if os.path.exists(cfg_path):
            cfg = json.load(open(cfg_path, encoding="utf-8"))
            lowercase = bool(cfg.get("do_lower_case", True))
            strip = cfg.get("strip_accents")
            chinese = bool(cfg.get("tokenize_chinese_chars", True))
        vocab_path = os.path.join(path, "vocab.txt")
        if os.path.exists(vocab_path):
            vocab = [line.rstrip("\n") for line in open(vocab_path, encoding="utf-8")]
            tj_path = os.path.join(path, "tokenizer.json")
            if os.path.exists(tj_path):  # the specials' names are written there only (MPNet ships both files)
                tj = json.load(open(tj_path, encoding="utf-8"))
                if tj.get("post_processor") is not None and (tj.get("model") or {}).get("type") == "WordPiece":
                    specials = wordpiece_specials(tj)
        else:
            tj = json.load(open(os.path.join(path, "tokenizer.json"), encoding="utf-8"))
            if tj["model"]["type"] != "WordPiece":
                raise ValueError(f"tokenizer model {tj['model']['type']} is not WordPiece")
            vocab = [""] * (max(tj["model"]["vocab"].values()) + 1)
            for tok, i in tj["model"]["vocab"].items():
                vocab[i] = tok
            norm = tj.get("normalizer") or {}
            if norm.get("type") == "BertNormalizer":
                lowercase = bool(norm.get("lowercase", True))
                strip = norm.get("strip_accents")
                chinese = bool(norm.get("handle_chinese_chars", True))
                clean = bool(norm.get("clean_text", True))
            if tj.get("post_processor") is not None:  # (none: the [CLS] ... [SEP] this tokenizer has always added)
                specials = wordpiece_specials(tj)
        return cls(vocab, lowercase, strip, chinese, clean, max_length, specials)

    def encode_batch(self, texts: list[str]) -> tuple[np.ndarray, np.ndarray]:
        """-> (ids int32[total], offsets int64[n + 1]); every sequence is [CLS] ... [SEP]."""
        n = len(texts)
        raw = [t.encode("utf-8", "replace") for t in texts]
        arr = (C.c_char_p * max(n, 1))(*raw)
        lens = np.asarray([len(b) for b in raw], np.int64)
        off = np.zeros(n + 1, np.int64)
        cap = int(sum(min(len(b) + 2, self.max_length) for b in raw)) + 2  # a piece consumes >= 1 byte
        ids = np.empty(cap, np.int32)
        needed = C.c_int64()
        rc = self._lib.vr_wordpiece_encode(self._h, arr, lens.ctypes.data_as(C.POINTER(C.c_int64)), n, self.max_length,
                                           off.ctypes.data_as(C.POINTER(C.c_int64)), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                           cap, C.byref(needed))
        check(rc)
        return ids[: int(needed.value)].copy(), off

    def encode_pairs(self, a_texts: list[str], b_texts: list[str]) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Cross-encoder input: sequence i is [CLS] a_i [SEP] b_i [SEP], truncated LongestFirst to max_length ids.
        -> (ids int32[total], offsets int64[n + 1], seg_b int32[n]: the position of each sequence's first segment-B id)."""
        if self.specials[:2] != DEFAULT_SPECIALS[:2]:
            raise ValueError(f"encode_pairs on a tokenizer with the specials {self.specials[0]!r} / {self.specials[1]!r}: "
                             "its model pairs with another template than [CLS] A [SEP] B [SEP] (MPNet cross-encoders "
                             "are not implemented)")
        n = len(a_texts)
        if len(b_texts) != n:
            raise ValueError(f"{n} first texts, {len(b_texts)} second texts")
        ra = [t.encode("utf-8", "replace") for t in a_texts]
        rb = [t.encode("utf-8", "replace") for t in b_texts]
        aa = (C.c_char_p * max(n, 1))(*ra)
        ba = (C.c_char_p * max(n, 1))(*rb)
        al = np.asarray([len(b) for b in ra] or [0], np.int64)
        bl = np.asarray([len(b) for b in rb] or [0], np.int64)
        off = np.zeros(n + 1, np.int64)
        seg = np.zeros(max(n, 1), np.int32)
        cap = n * self.max_length
        ids = np.empty(max(cap, 1), np.int32)
        needed = C.c_int64()
        p64 = C.POINTER(C.c_int64)
        p32 = C.POINTER(C.c_int32)
        check(self._lib.vr_wordpiece_encode_pairs(self._h, aa, al.ctypes.data_as(p64), ba, bl.ctypes.data_as(p64), n,
                                                  self.max_length, off.ctypes.data_as(p64), ids.ctypes.data_as(p32),
                                                  seg.ctypes.data_as(p32), cap, C.byref(needed)))
        return ids[: int(needed.value)].copy(), off, seg[:n].copy()
