"""Semantic chunking, host side: from documents to the sequences and UNIT spans ``encode_semantic``
takes, and from its ``unit_start`` back to chunks. Pure host code, no GPU.

A unit is a sentence-sized piece of the document: the native chunker's ``sentence`` strategy at
VOITTA_SEMANTIC_UNIT_CHARS characters, overlap 0 — no new splitter. ``late_chunking.plan`` with the units in the chunks'
place gives the sequences, the windows of a long document and the unit spans unchanged; a chunk never crosses a window,
because a window is a sequence. The device joins neighbouring units into chunks and returns one late-chunked row per
chunk; ``rebuild`` turns its ``unit_start`` into ``(text, start_char, end_char)``: the document from the first unit's
located start to the last unit's located end.

A document whose plan is None (a unit that is not found, or without tokens), or whose located units are not in order (or more
than 2048 in one window),
is chunked and embedded the plain way by the caller; ``plan_units`` says which."""
from __future__ import annotations

import re
from dataclasses import dataclass, field

import numpy as np

from . import late_chunking as _late


@dataclass
class UnitPlan:
    plan: _late.Plan                # of the documents in `planned`, back to back: span_off / span_tok are the units
    planned: list = field(default_factory=list)  # indices (into the documents given) of the documents in the plan
    where: list = field(default_factory=list)    # per planned document: the (start, end) characters of its units
    plain: list = field(default_factory=list)    # indices of the documents that go the plain way


MAX_UNITS_PER_SEQUENCE = 2048  # vr_encode_semantic's limit


def _usable(p: _late.Plan) -> bool:
    """Inside every sequence (window) of a document's plan the units are in order, never overlap and are at most 2048."""
    for i in range(p.n_seq):
        tok = p.span_tok[int(p.span_off[i]):int(p.span_off[i + 1])]
        if len(tok) > MAX_UNITS_PER_SEQUENCE:
            return False
        if len(tok) > 1 and not np.all(tok[1:, 0] >= tok[:-1, 1]):
            return False
    return True


def anchor_units(document: str, unit_texts) -> list | None:
    """The units as verbatim slices of the document, or None when one is not found. The ``sentence`` strategy joins the
    sentences it packs into a unit with one space, whatever separated them (a paragraph break, two spaces): a unit is
    found as its words in order with any whitespace between them, at or after the end of the unit before it."""
    out, pos = [], 0
    for t in unit_texts:
        words = t.split()
        m = re.compile(r"\s+".join(map(re.escape, words))).search(document, pos) if words else None
        if m is None:
            return None
        out.append(document[m.start():m.end()])
        pos = m.end()
    return out


def plan_units(documents, tokenize, max_tokens: int, context: int, prefix_ids=(), lead: int = 1) -> UnitPlan:
    """documents: [(text, unit_texts)]. Every document whose units are found in it (``anchor_units``) and that
    ``late_chunking.plan`` can plan with them in order is in the plan; the others (and those without units) are listed
    in ``plain``."""
    out, plans = UnitPlan(_late.concat([])), []
    for k, (text, unit_texts) in enumerate(documents):
        unit_texts = anchor_units(text, unit_texts) or []
        p = _late.plan(text, unit_texts, tokenize, max_tokens, context, prefix_ids, lead) if unit_texts else None
        if p is None or not _usable(p):
            out.plain.append(k)
            continue
        plans.append(p)
        out.planned.append(k)
        out.where.append(_late.locate(text, unit_texts))
    out.plan = _late.concat(plans)
    return out


def rebuild(text: str, where: list, unit_start) -> list:
    """[(chunk text, start_char, end_char)] of one document from its units' located positions and their start flags."""
    first = [r for r, s in enumerate(unit_start) if s]
    if len(where) != len(unit_start) or (where and first[:1] != [0]):
        raise ValueError(f"{len(where)} units, {len(unit_start)} start flags, first start at {first[:1]}")
    out = []
    for a, b in zip(first, first[1:] + [len(where)]):
        start, end = where[a][0], where[b - 1][1]
        out.append((text[start:end], start, end))
    return out


# ---- the per-file drop-in sequence: chunk_text -> embed_texts -> store_chunks --------------------------------------

class SemanticDocument:
    """What the chunks of one document share: how many they are, and their vectors, one row each."""

    __slots__ = ("n_chunks", "vectors")

    def __init__(self, vectors: np.ndarray):
        self.n_chunks = int(vectors.shape[0])
        self.vectors = vectors


class SemanticChunkText(str):
    """A chunk text that carries its document's vectors (``sem_doc``) and its index among them (``sem_index``); a plain
    ``str`` everywhere else, as ``late_chunking.LateChunkText`` is."""

    __slots__ = ("sem_doc", "sem_index")

    def __new__(cls, text: str, doc: SemanticDocument, index: int):
        self = super().__new__(cls, text)
        self.sem_doc = doc
        self.sem_index = index
        return self

    def __reduce__(self):  # pickles and copies as its characters alone
        return (str, (str(self),))


def wrap_chunks(chunk_texts, vectors: np.ndarray) -> list:
    doc = SemanticDocument(vectors)
    assert doc.n_chunks == len(chunk_texts)
    return [SemanticChunkText(t, doc, i) for i, t in enumerate(chunk_texts)]


def carried_vectors(texts) -> np.ndarray | None:
    """The carried rows, in order, when ``texts`` is made of complete documents — every element a SemanticChunkText, the
    elements of each document that document's chunks in order — and None for anything else."""
    rows, i, n = [], 0, len(texts)
    if n == 0:
        return None
    while i < n:
        first = texts[i]
        if type(first) is not SemanticChunkText or first.sem_index != 0:
            return None
        doc = first.sem_doc
        if i + doc.n_chunks > n:
            return None
        for k in range(doc.n_chunks):
            t = texts[i + k]
            if type(t) is not SemanticChunkText or t.sem_doc is not doc or t.sem_index != k:
                return None
        rows.append(doc.vectors)
        i += doc.n_chunks
    return np.concatenate(rows)
