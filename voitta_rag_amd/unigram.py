"""SentencePiece Unigram tokenizer through the C-ABI (vr_unigram_*, csrc/unigram.cpp): the tokenise step of the
XLM-RoBERTa models (intfloat/multilingual-e5-*, BAAI/bge-reranker-*) as HF tokenizers runs it from their
tokenizer.json. Same surface as WordPieceTokenizer: packed ids + offsets, the form vr_encode / vr_index_batch take.

``from_pretrained`` accepts the XLM-R pipeline only (see ``parse_tokenizer_json``) and raises ValueError for anything
else, so that a caller can fall back to the tokenizers library."""
from __future__ import annotations

import base64
import ctypes as C
import json
import os

import numpy as np

from ._lib import check, load_library

VR_UNIGRAM_PRE_METASPACE = 0
VR_UNIGRAM_PRE_WHITESPACE_METASPACE = 1
PREPEND = {"always": 0, "first": 1, "never": 2}
VR_ADDED_LSTRIP, VR_ADDED_RSTRIP, VR_ADDED_SINGLE_WORD = 1, 2, 4
META = "▁"


def _metaspace(pt: dict) -> int:
    if pt.get("replacement", META) != META:
        raise ValueError(f"Metaspace replacement {pt.get('replacement')!r}")
    if not pt.get("split", True):
        raise ValueError("Metaspace with split=false")
    if "prepend_scheme" in pt:
        scheme = pt["prepend_scheme"]
    else:  # older files
        scheme = "always" if pt.get("add_prefix_space", True) else "never"
    if scheme not in PREPEND:
        raise ValueError(f"Metaspace prepend_scheme {scheme!r}")
    return PREPEND[scheme]


def _special_id(spec: dict, tok: str) -> int:
    st = spec.get(tok)
    if st is None or len(st.get("ids", [])) != 1:
        raise ValueError(f"template special token {tok!r} is not one id")
    return int(st["ids"][0])


def parse_tokenizer_json(spec: dict) -> dict:
    """The create arguments of vr_unigram_create from a parsed tokenizer.json, or ValueError for a pipeline outside
    the XLM-R shape: Unigram (no byte fallback); normalizer null, Precompiled, or Sequence[Precompiled,
    Replace(" {2,}", " ")]; pre-tokenizer Metaspace or Sequence[WhitespaceSplit, Metaspace]; TemplateProcessing
    "<s> $A </s>" / "<s> $A </s> </s> $B </s>", "$A </s>" (T5: bos_id -1) or RobertaProcessing; added tokens with
    normalized=false."""
    model = spec.get("model") or {}
    if model.get("type") != "Unigram":
        raise ValueError(f"tokenizer model {model.get('type')} is not Unigram")
    if model.get("byte_fallback"):
        raise ValueError("Unigram with byte_fallback is not implemented")
    if model.get("unk_id") is None:
        raise ValueError("Unigram without an unk_id")
    vocab = model["vocab"]
    pieces = [p for p, _ in vocab]
    scores = np.asarray([float(s) for _, s in vocab], np.float64)
    # ---- normalizer
    norm = spec.get("normalizer")
    steps = [] if norm is None else (norm["normalizers"] if norm.get("type") == "Sequence" else [norm])
    charsmap, replace = b"", False
    for k, st in enumerate(steps):
        if st.get("type") == "Precompiled" and k == 0:
            raw = st.get("precompiled_charsmap")
            charsmap = base64.b64decode(raw) if raw else b""
        elif (st.get("type") == "Replace" and st.get("pattern") == {"Regex": " {2,}"} and st.get("content") == " "
              and k == len(steps) - 1 and not replace):
            replace = True
        else:
            raise ValueError(f"normalizer step {st.get('type')} is not part of the XLM-R pipeline")
    # ---- pre-tokenizer
    pt = spec.get("pre_tokenizer") or {}
    if pt.get("type") == "Metaspace":
        pre, prepend = VR_UNIGRAM_PRE_METASPACE, _metaspace(pt)
    elif (pt.get("type") == "Sequence" and [p.get("type") for p in pt.get("pretokenizers", [])]
          == ["WhitespaceSplit", "Metaspace"]):
        pre, prepend = VR_UNIGRAM_PRE_WHITESPACE_METASPACE, _metaspace(pt["pretokenizers"][1])
    else:
        raise ValueError(f"pre-tokenizer {pt.get('type')} is not Metaspace or Sequence[WhitespaceSplit, Metaspace]")
    # ---- post-processor
    post = spec.get("post_processor") or {}
    if post.get("type") == "RobertaProcessing":
        bos, eos = int(post["cls"][1]), int(post["sep"][1])
    elif post.get("type") == "TemplateProcessing":
        def shape(items):
            out = []
            for it in items:
                if "SpecialToken" in it:
                    out.append(it["SpecialToken"]["id"])
                else:
                    out.append("$" + it["Sequence"]["id"])
            return out

        single, pair = shape(post["single"]), shape(post.get("pair") or [])
        if len(single) == 2 and single[0] == "$A" and not single[1].startswith("$"):
            # T5: $A </s> (its pair template, $A </s> $B </s>, is not implemented: encode_pairs is refused). bos -1 = none
            bos = -1
            eos = _special_id(post.get("special_tokens") or {}, single[1])
        elif len(single) != 3 or single[1] != "$A" or pair != [single[0], "$A", single[2], single[2], "$B", single[2]]:
            raise ValueError(f"post-processor template {single} / {pair} is not <s> $A </s> / <s> $A </s> </s> $B </s> "
                             "(or $A </s>)")
        else:
            bos = _special_id(post.get("special_tokens") or {}, single[0])
            eos = _special_id(post.get("special_tokens") or {}, single[2])
    else:
        raise ValueError(f"post-processor {post.get('type')} is not TemplateProcessing or RobertaProcessing")
    # ---- added tokens
    added, added_ids, added_flags = [], [], []
    for at in spec.get("added_tokens") or []:
        if at.get("normalized", not at.get("special", False)):
            raise ValueError(f"added token {at.get('content')!r} is matched after normalisation")
        added.append(at["content"])
        added_ids.append(int(at["id"]))
        added_flags.append((VR_ADDED_LSTRIP if at.get("lstrip") else 0) | (VR_ADDED_RSTRIP if at.get("rstrip") else 0)
                           | (VR_ADDED_SINGLE_WORD if at.get("single_word") else 0))
    n = len(pieces)
    for name, i in (("unk", model["unk_id"]), ("bos", bos), ("eos", eos)):
        if not 0 <= int(i) < n and not (name == "bos" and i == -1):
            raise ValueError(f"{name} id {i} outside the {n} pieces")
    return dict(pieces=pieces, scores=scores, unk_id=int(model["unk_id"]), bos_id=bos, eos_id=eos, charsmap=charsmap,
                replace_spaces=replace, pre_tokenizer=pre, prepend_scheme=prepend, added=added, added_ids=added_ids,
                added_flags=added_flags)


def is_unigram_pipeline(spec: dict) -> bool:
    try:
        parse_tokenizer_json(spec)
        return True
    except (ValueError, KeyError, TypeError):
        return False


class UnigramTokenizer:
    def __init__(self, pieces: list[str], scores, unk_id: int, bos_id: int, eos_id: int, charsmap: bytes = b"",
                 replace_spaces: bool = False, pre_tokenizer: int = VR_UNIGRAM_PRE_METASPACE, prepend_scheme: int = 0,
                 added: list[str] = (), added_ids: list[int] = (), added_flags: list[int] = (), max_length: int = 512):
        self._lib = load_library()
        self.vocab_size = len(pieces)
        self.bos_id = int(bos_id)  # -1: the template is $A </s>
        self.max_length = int(max_length)
        raw = [p.encode("utf-8") for p in pieces]
        arr = (C.c_char_p * len(raw))(*raw)
        sc = np.ascontiguousarray(scores, np.float64)
        cm = (C.c_uint8 * max(len(charsmap), 1)).from_buffer_copy(charsmap or b"\0")
        na = len(added)
        at = (C.c_char_p * max(na, 1))(*[a.encode("utf-8") for a in added])
        ai = np.asarray(list(added_ids) or [0], np.int32)
        af = np.asarray(list(added_flags) or [0], np.int32)
        h = C.c_void_p()
        check(self._lib.vr_unigram_create(arr, sc.ctypes.data_as(C.POINTER(C.c_double)), len(raw), unk_id, bos_id, eos_id,
                                          cm, len(charsmap), int(replace_spaces), pre_tokenizer, prepend_scheme, at,
                                          ai.ctypes.data_as(C.POINTER(C.c_int32)), af.ctypes.data_as(C.POINTER(C.c_int32)),
                                          na, C.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.vr_unigram_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def from_tokenizer_json(cls, spec: dict, max_length: int = 512) -> "UnigramTokenizer":
        return cls(**parse_tokenizer_json(spec), max_length=max_length)

    @classmethod
    def from_pretrained(cls, path: str, max_length: int = 512) -> "UnigramTokenizer":
        """tokenizer.json of an XLM-R checkpoint directory; ValueError for any other pipeline."""
        tj = os.path.join(path, "tokenizer.json")
        if not os.path.exists(tj):
            raise ValueError(f"no tokenizer.json under {path}")
        return cls.from_tokenizer_json(json.load(open(tj, encoding="utf-8")), max_length)

    def encode_batch(self, texts: list[str]) -> tuple[np.ndarray, np.ndarray]:
        """-> (ids int32[total], offsets int64[n + 1]); every sequence is <s> ... </s> (a T5 tokenizer: ... </s>)."""
        n = len(texts)
        raw = [t.encode("utf-8", "replace") for t in texts]
        arr = (C.c_char_p * max(n, 1))(*raw)
        lens = np.asarray([len(b) for b in raw] or [0], np.int64)
        off = np.zeros(n + 1, np.int64)
        # every sequence holds at most max_length ids after truncation; no bound by the byte count holds here (the
        # Metaspace U+2581 consumes no input byte, and the charsmap may expand a code point into several)
        cap = max(n, 1) * self.max_length
        ids = np.empty(cap, np.int32)
        needed = C.c_int64()
        check(self._lib.vr_unigram_encode(self._h, arr, lens.ctypes.data_as(C.POINTER(C.c_int64)), n, self.max_length,
                                          off.ctypes.data_as(C.POINTER(C.c_int64)), ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                          cap, C.byref(needed)))
        return ids[: int(needed.value)].copy(), off

    def encode_pairs(self, a_texts: list[str], b_texts: list[str]) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Cross-encoder input: sequence i is <s> a_i </s> </s> b_i </s>, truncated LongestFirst to max_length ids.
        -> (ids int32[total], offsets int64[n + 1], seg_b int32[n]: the position of each sequence's first id of b_i)."""
        n = len(a_texts)
        if self.bos_id < 0:
            raise ValueError("encode_pairs on a tokenizer whose template is $A </s> (T5): it has no pair template here")
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
        check(self._lib.vr_unigram_encode_pairs(self._h, aa, al.ctypes.data_as(p64), ba, bl.ctypes.data_as(p64), n,
                                                self.max_length, off.ctypes.data_as(p64), ids.ctypes.data_as(p32),
                                                seg.ctypes.data_as(p32), cap, C.byref(needed)))
        return ids[: int(needed.value)].copy(), off, seg[:n].copy()
