"""Byte-level BPE tokenizer through the C-ABI (vr_bpe_*, csrc/bpe.cpp): the tokenise step of the ModernBERT models
(gte-modernbert-base, modernbert-embed-base, gte-reranker-modernbert-base) as HF tokenizers runs it from their
tokenizer.json. Same surface as UnigramTokenizer: packed ids + offsets, the form vr_encode / vr_index_batch take.

``from_pretrained`` accepts one pipeline only (see ``parse_tokenizer_json``) and raises ValueError naming the offending
field for anything else, so that a caller can fall back to the tokenizers library."""
from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

from ._lib import check, load_library

VR_ADDED_LSTRIP, VR_ADDED_RSTRIP, VR_ADDED_SINGLE_WORD, VR_ADDED_NORMALIZED = 1, 2, 4, 8


def _special_id(spec: dict, tok: str) -> int:
    st = spec.get(tok)
    if st is None or len(st.get("ids", [])) != 1:
        raise ValueError(f"post_processor: template special token {tok!r} is not one id")
    return int(st["ids"][0])


def parse_tokenizer_json(spec: dict) -> dict:
    """The create arguments of vr_bpe_create from a parsed tokenizer.json, or ValueError for a pipeline outside this
    one: model BPE with dropout null, no continuing_subword_prefix or end_of_word_suffix, byte_fallback and
    ignore_merges false, fuse_unk false when there is an unk_token; normalizer null or NFC; pre-tokenizer
    ByteLevel(add_prefix_space=false, use_regex=true); TemplateProcessing "cls $A sep" / "cls $A sep $B sep"."""
    model = spec.get("model") or {}
    if model.get("type") != "BPE":
        raise ValueError(f"model.type {model.get('type')!r} is not BPE")
    if model.get("dropout") is not None:
        raise ValueError(f"model.dropout {model['dropout']} is not implemented (null only)")
    for key in ("continuing_subword_prefix", "end_of_word_suffix"):
        if model.get(key):
            raise ValueError(f"model.{key} {model[key]!r} is not implemented")
    for key in ("byte_fallback", "ignore_merges"):
        if model.get(key):
            raise ValueError(f"model.{key} true is not implemented")
    vocab_map = model["vocab"]
    n = max(vocab_map.values()) + 1
    for at in spec.get("added_tokens") or []:
        n = max(n, int(at["id"]) + 1)
    vocab = [None] * n
    for tok, i in vocab_map.items():
        vocab[i] = tok
    unk = model.get("unk_token")
    if unk is not None:
        if unk not in vocab_map:
            raise ValueError(f"model.unk_token {unk!r} is not in the vocabulary")
        if model.get("fuse_unk"):
            raise ValueError("model.fuse_unk true is not implemented")
    merges = [tuple(m.split(" ", 1)) if isinstance(m, str) else tuple(m) for m in model.get("merges") or []]
    if any(len(m) != 2 for m in merges):
        raise ValueError("model.merges holds an entry that is not a pair")
    norm = spec.get("normalizer")
    if norm is not None and norm.get("type") != "NFC":
        raise ValueError(f"normalizer {norm.get('type')!r} is not implemented (NFC or none)")
    pt = spec.get("pre_tokenizer") or {}
    if pt.get("type") != "ByteLevel":
        raise ValueError(f"pre_tokenizer {pt.get('type')!r} is not ByteLevel")
    if pt.get("add_prefix_space", True):
        raise ValueError("pre_tokenizer.add_prefix_space true is not implemented")
    if not pt.get("use_regex", True):
        raise ValueError("pre_tokenizer.use_regex false is not implemented")
    post = spec.get("post_processor") or {}
    if post.get("type") != "TemplateProcessing":
        raise ValueError(f"post_processor {post.get('type')!r} is not TemplateProcessing")

    def shape(items):
        return [it["SpecialToken"]["id"] if "SpecialToken" in it else "$" + it["Sequence"]["id"] for it in items]

    single, pair = shape(post["single"]), shape(post.get("pair") or [])
    if len(single) != 3 or single[1] != "$A" or pair != [single[0], "$A", single[2], "$B", single[2]]:
        raise ValueError(f"post_processor template {single} / {pair} is not cls $A sep / cls $A sep $B sep")
    cls_id = _special_id(post.get("special_tokens") or {}, single[0])
    sep_id = _special_id(post.get("special_tokens") or {}, single[2])
    added, added_ids, added_flags = [], [], []
    for at in spec.get("added_tokens") or []:
        if vocab[int(at["id"])] is None:
            vocab[int(at["id"])] = at["content"]
        added.append(at["content"])
        added_ids.append(int(at["id"]))
        added_flags.append((VR_ADDED_LSTRIP if at.get("lstrip") else 0) | (VR_ADDED_RSTRIP if at.get("rstrip") else 0)
                           | (VR_ADDED_SINGLE_WORD if at.get("single_word") else 0)
                           | (VR_ADDED_NORMALIZED if at.get("normalized", not at.get("special", False)) else 0))
    if any(v is None for v in vocab):
        raise ValueError("model.vocab has an id without a token")
    for name, i in (("cls", cls_id), ("sep", sep_id)):
        if not 0 <= i < n:
            raise ValueError(f"post_processor: {name} id {i} outside the {n} tokens")
    return dict(vocab=vocab, merges=merges, unk_id=-1 if unk is None else int(vocab_map[unk]), cls_id=cls_id, sep_id=sep_id,
                nfc=norm is not None, added=added, added_ids=added_ids, added_flags=added_flags)


class BpeTokenizer:
    def __init__(self, vocab: list[str], merges: list[tuple[str, str]], unk_id: int, cls_id: int, sep_id: int,
                 nfc: bool = False, added: list[str] = (), added_ids: list[int] = (), added_flags: list[int] = (),
                 max_length: int = 512):
        self._lib = load_library()
        self.vocab_size = len(vocab)
        self.max_length = int(max_length)
        va = (C.c_char_p * len(vocab))(*[v.encode("utf-8") for v in vocab])
        nm = len(merges)
        ml = (C.c_char_p * max(nm, 1))(*[m[0].encode("utf-8") for m in merges])
        mr = (C.c_char_p * max(nm, 1))(*[m[1].encode("utf-8") for m in merges])
        na = len(added)
        at = (C.c_char_p * max(na, 1))(*[a.encode("utf-8") for a in added])
        ai = np.asarray(list(added_ids) or [0], np.int32)
        af = np.asarray(list(added_flags) or [0], np.int32)
        h = C.c_void_p()
        p32 = C.POINTER(C.c_int32)
        check(self._lib.vr_bpe_create(va, len(vocab), ml, mr, nm, int(unk_id), int(cls_id), int(sep_id), int(bool(nfc)), at,
                                      ai.ctypes.data_as(p32), af.ctypes.data_as(p32), na, C.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.vr_bpe_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def from_tokenizer_json(cls, spec: dict, max_length: int = 512) -> "BpeTokenizer":
        return cls(**parse_tokenizer_json(spec), max_length=max_length)

    @classmethod
    def from_pretrained(cls, path: str, max_length: int = 512) -> "BpeTokenizer":
        """tokenizer.json of a ModernBERT checkpoint directory; ValueError for any other pipeline."""
        tj = os.path.join(path, "tokenizer.json")
        if not os.path.exists(tj):
            raise ValueError(f"no tokenizer.json under {path}")
        return cls.from_tokenizer_json(json.load(open(tj, encoding="utf-8")), max_length)

    def encode(self, texts: list[str], capacity: int | None = None) -> tuple[np.ndarray, np.ndarray]:
        """-> (ids int32[total], offsets int64[n + 1]); every sequence is cls ... sep, at most max_length ids."""
        n = len(texts)
        raw = [t if isinstance(t, bytes) else t.encode("utf-8", "replace") for t in texts]
        arr = (C.c_char_p * max(n, 1))(*raw)
        lens = np.asarray([len(b) for b in raw] or [0], np.int64)
        off = np.zeros(n + 1, np.int64)
        cap = max(n, 1) * self.max_length if capacity is None else int(capacity)
        ids = np.empty(max(cap, 1), np.int32)
        needed = C.c_int64()
        p64 = C.POINTER(C.c_int64)
        check(self._lib.vr_bpe_encode(self._h, arr, lens.ctypes.data_as(p64), n, self.max_length, off.ctypes.data_as(p64),
                                      ids.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(needed)))
        return ids[: int(needed.value)].copy(), off

    encode_batch = encode  # (the name NativeSentenceEncoder.tokenize calls)

    def encode_pairs(self, a_texts: list[str], b_texts: list[str]) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Cross-encoder input: sequence i is cls a_i sep b_i sep, truncated LongestFirst to max_length ids.
        -> (ids int32[total], offsets int64[n + 1], seg_b int32[n]: the position of each sequence's first id of b_i)."""
        n = len(a_texts)
        if len(b_texts) != n:
            raise ValueError(f"{n} first texts, {len(b_texts)} second texts")
        ra = [t if isinstance(t, bytes) else t.encode("utf-8", "replace") for t in a_texts]
        rb = [t if isinstance(t, bytes) else t.encode("utf-8", "replace") for t in b_texts]
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
        check(self._lib.vr_bpe_encode_pairs(self._h, aa, al.ctypes.data_as(p64), ba, bl.ctypes.data_as(p64), n,
                                            self.max_length, off.ctypes.data_as(p64), ids.ctypes.data_as(p32),
                                            seg.ctypes.data_as(p32), cap, C.byref(needed)))
        return ids[: int(needed.value)].copy(), off, seg[:n].copy()
