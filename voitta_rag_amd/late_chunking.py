"""Late chunking, host side: from a document and its chunks to the token sequences and token spans that
``encode_spans`` / ``index_batch_spans`` take. Pure host code, no GPU.

The document goes through the encoder once (or, when it is longer than the model's window, in a few windows that
each carry left context) and every chunk's vector is the mean of the final hidden states of the chunk's own tokens.
``plan`` is deterministic:

1. every chunk is LOCATED in the document: chunk j is the first occurrence of its text at or after the located start
   of chunk j - 1 (chunk 0 from position 0). The chunker's ``start_char`` is not used: for overlapped chunks the
   reference does not advance it (include/voitta_engine.h, vr_chunk_texts). A chunk that is not found: ``None``, the
   caller encodes the document's chunks the plain way;
2. the located starts and ends of all chunks, with 0 and len(document), cut the document into SEGMENTS. Each non-blank
   segment is tokenised on its own (specials removed; the tokenizer's own limit applies to a segment); the document's
   token sequence is the concatenation. A chunk's token span is the union of the segments inside it — exact, because
   every chunk boundary is a segment boundary. Where the chunker cut inside a word, that word is tokenised as two
   pieces (the chunk's own text starts with such a fragment too). A chunk without tokens: ``None``;
3. L = max_tokens - 2 - len(prefix_ids). A document of at most L tokens is one sequence. A longer one is cut greedily
   over the chunk list into WINDOWS: a window starts ``context`` tokens before the first token of its first chunk
   (clamped to 0), takes following chunks while end(chunk) - window_start <= L, and ends at the end of the last chunk
   taken (the document's last window also takes the trailing tokens, as many as still fit in L). A chunk that alone exceeds
   L - context gets the left context that still fits; one that alone exceeds L is truncated at the window's end and
   flagged;
4. each window becomes bos, prefix_ids, the window's tokens, eos; spans are shifted by 1 + len(prefix_ids), so they
   never cover specials or the prefix. (A tokenizer without a bos — T5's "$A </s>" — is planned with lead=0: no bos.)

``tokenize(texts)`` is the model's: a list of strings -> packed (ids, offsets) WITH the two specials around every
text, as ``NativeSentenceEncoder.tokenize`` returns them; bos and eos are read off its output."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np


@dataclass
class Plan:
    """Sequences and spans ready for ``encode_spans`` / ``index_batch_spans``: row r of ``span_tok`` is chunk r."""

    ids: np.ndarray        # int32, the sequences back to back
    offsets: np.ndarray    # int32 [n_seq + 1]
    span_off: np.ndarray   # int32 [n_seq + 1]: the chunks (rows of span_tok) of each sequence
    span_tok: np.ndarray   # int32 [n_chunks, 2]: (begin, end) token positions inside the chunk's own sequence
    truncated: np.ndarray  # bool [n_chunks]: the chunk alone exceeded the window, its span was cut at the window's end
    late: list = field(default_factory=list)  # plan_many: per document, False = its chunks went the plain way

    @property
    def n_seq(self) -> int:
        return int(self.offsets.shape[0]) - 1

    @property
    def n_chunks(self) -> int:
        return int(self.span_tok.shape[0])

    def spans(self):
        """(n_seq, span_off, span_tok): the ``spans`` argument of ``VectorStoreService.index_chunks``."""
        return self.n_seq, self.span_off, self.span_tok


def locate(document: str, chunk_texts) -> list | None:
    """(start, end) character positions of every chunk in the document, or None when one is not found (or is empty)."""
    out, pos = [], 0
    for text in chunk_texts:
        i = document.find(text, pos) if text else -1
        if i < 0:
            return None
        out.append((i, i + len(text)))
        pos = i
    return out


def strip_specials(ids, off, lead: int = 1):
    """Packed (ids, offsets) with specials -> the list of id arrays without them, and (bos, eos) (None without texts).
    lead: the number of specials in front of a text, 1 — or 0 for a tokenizer whose template is "$A </s>" (T5), whose
    bos is then None."""
    ids, off = np.asarray(ids), np.asarray(off)
    pieces = [ids[int(off[i]) + lead: int(off[i + 1]) - 1] for i in range(off.shape[0] - 1)]
    specials = (int(ids[0]) if lead else None, int(ids[int(off[1]) - 1])) if off.shape[0] > 1 else None
    return pieces, specials


def prefix_ids_of(prefix: str, tokenize, lead: int = 1) -> tuple:
    """The ids of a passage prefix ('passage: ', VOITTA_EMBED_PASSAGE_PREFIX), tokenised once without specials."""
    if not prefix.strip():
        return ()
    pieces, _ = strip_specials(*tokenize([prefix]), lead)
    return tuple(int(t) for t in pieces[0])


def plan(document: str, chunk_texts, tokenize, max_tokens: int, context: int, prefix_ids=(), lead: int = 1) -> Plan | None:
    """lead: the specials in front of a text (strip_specials): 1, or 0 for a tokenizer without a bos."""
    chunk_texts = list(chunk_texts)
    prefix = [int(t) for t in prefix_ids]
    L = int(max_tokens) - (lead + 1) - len(prefix)
    if L < 1:
        raise ValueError(f"max_tokens={max_tokens} leaves no room for text beside {lead + 1} specials and {len(prefix)} prefix ids")
    if context < 0:
        raise ValueError(f"context={context} must not be negative")
    where = locate(document, chunk_texts)
    if not where:
        return None
    # segments: every chunk boundary is a segment boundary
    cuts = sorted({0, len(document)} | {p for se in where for p in se})
    index_of = {c: k for k, c in enumerate(cuts)}
    segments = [document[a:b] for a, b in zip(cuts, cuts[1:])]
    live = [k for k, s in enumerate(segments) if s.strip()]
    if not live:
        return None
    pieces, specials = strip_specials(*tokenize([segments[k] for k in live]), lead)
    bos, eos = specials
    tok_at = np.zeros(len(cuts), np.int64)  # first token of the segment that starts at cuts[k]
    counts = np.zeros(len(segments), np.int64)
    counts[live] = [len(p) for p in pieces]
    tok_at[1:] = np.cumsum(counts)
    tokens = np.concatenate(pieces).astype(np.int32) if pieces else np.zeros(0, np.int32)
    N = int(tok_at[-1])
    cb = [int(tok_at[index_of[s]]) for s, _ in where]
    ce = [int(tok_at[index_of[e]]) for _, e in where]
    if any(e <= b for b, e in zip(cb, ce)):
        return None  # a chunk without tokens
    n = len(where)
    # windows: (token start, token end, first chunk, one past the last chunk)
    windows = []
    if N <= L:
        windows.append((0, N, 0, n))
    else:
        j = 0
        while j < n:
            ws = max(0, cb[j] - context)
            if ce[j] - ws > L:  # the chunk alone exceeds L - context: the left context that still fits
                ws = min(cb[j], ce[j] - L)
            we = min(ce[j], ws + L)
            k = j + 1
            while k < n and ce[k] - ws <= L:
                we = max(we, ce[k])
                k += 1
            if k == n:
                we = max(we, min(N, ws + L))  # the document's trailing tokens, as far as the window holds them
            windows.append((ws, we, j, k))
            j = k
    shift = lead + len(prefix)
    ids, offsets, span_off = [], [0], [0]
    span_tok = np.zeros((n, 2), np.int32)
    truncated = np.zeros(n, bool)
    head, tail = np.asarray(([bos] if lead else []) + prefix, np.int32), np.asarray([eos], np.int32)
    for ws, we, j, k in windows:
        ids += [head, tokens[ws:we], tail]
        offsets.append(offsets[-1] + shift + (we - ws) + 1)
        span_off.append(k)
        for c in range(j, k):
            span_tok[c] = (cb[c] - ws + shift, min(ce[c], we) - ws + shift)
            truncated[c] = ce[c] > we
    return Plan(np.concatenate(ids), np.asarray(offsets, np.int32), np.asarray(span_off, np.int32), span_tok, truncated,
                [True])


def plain_plan(chunk_texts, tokenize, pooling: str = "mean") -> Plan:
    """The plain route as spans: every chunk text (as the plain route tokenises it, any prefix already in front) is a
    sequence of its own with one span that gives the vector of a plain call bit for bit — the whole sequence for a
    mean-pooled model, its first token for a [CLS]-pooled one (a mean over one row is that row)."""
    ids, off = tokenize(list(chunk_texts))
    ids, off = np.asarray(ids, np.int32), np.asarray(off, np.int32)
    n = off.shape[0] - 1
    lens = np.diff(off)
    first = np.maximum(lens - 1, 0) if pooling == "last" else np.zeros(n, np.int32)  # ("last": the span of the last token alone)
    span_tok = np.stack([first, np.ones(n, np.int32) if pooling == "cls" else lens], 1).astype(np.int32)
    return Plan(ids, off, np.arange(n + 1, dtype=np.int32), span_tok, np.zeros(n, bool), [False])


def concat(plans) -> Plan:
    """Plans back to back, chunk order kept."""
    plans = list(plans)
    if not plans:
        z = np.zeros(1, np.int32)
        return Plan(np.zeros(0, np.int32), z, z.copy(), np.zeros((0, 2), np.int32), np.zeros(0, bool), [])
    offsets, span_off, t, s = [np.zeros(1, np.int32)], [np.zeros(1, np.int32)], 0, 0
    for p in plans:
        offsets.append(p.offsets[1:] + t)
        span_off.append(p.span_off[1:] + s)
        t += int(p.offsets[-1])
        s += int(p.span_off[-1])
    return Plan(np.concatenate([p.ids for p in plans]).astype(np.int32), np.concatenate(offsets).astype(np.int32),
                np.concatenate(span_off).astype(np.int32), np.concatenate([p.span_tok for p in plans]).astype(np.int32),
                np.concatenate([p.truncated for p in plans]), [flag for p in plans for flag in p.late])


def plan_many(documents, tokenize, max_tokens: int, context: int, prefix_ids=(), plain_text=None,
              pooling: str = "mean", lead: int = 1) -> Plan:
    """``plan`` for a list of (document, chunk_texts), concatenated with chunk order kept across documents. A document
    whose plan is None goes the plain way inside the same result (``plain_plan`` of ``plain_text(chunk)``, the chunk as
    the plain route hands it to the tokenizer); ``late`` says which. Documents without chunks contribute nothing."""
    plans = []
    for document, chunk_texts in documents:
        chunk_texts = list(chunk_texts)
        if not chunk_texts:
            continue
        p = plan(document, chunk_texts, tokenize, max_tokens, context, prefix_ids, lead)
        if p is None:
            p = plain_plan([plain_text(t) if plain_text else t for t in chunk_texts], tokenize, pooling)
        plans.append(p)
    return concat(plans)


# ---- the per-file drop-in sequence: chunk_text -> embed_texts -> store_chunks --------------------------------------

class LateDocument:
    """What the chunks of one document share: its text and how many chunks it was cut into."""

    __slots__ = ("text", "n_chunks")

    def __init__(self, text: str, n_chunks: int):
        self.text = text
        self.n_chunks = n_chunks


class LateChunkText(str):
    """A chunk text that knows its document (``late_doc``) and its index in it (``late_index``); a plain ``str``
    everywhere else: it compares, hashes, slices, encodes and formats as one, and whatever is derived from it
    (a slice, a concatenation, an f-string) is a plain ``str`` again."""

    __slots__ = ("late_doc", "late_index")

    def __new__(cls, text: str, doc: LateDocument, index: int):
        self = super().__new__(cls, text)
        self.late_doc = doc
        self.late_index = index
        return self

    def __reduce__(self):  # pickles and copies as its characters alone
        return (str, (str(self),))


def wrap_chunks(document: str, chunk_texts) -> list:
    doc = LateDocument(document, len(chunk_texts))
    return [LateChunkText(t, doc, i) for i, t in enumerate(chunk_texts)]


def group_documents(texts) -> list | None:
    """[(document, chunk_texts)] when ``texts`` is made of complete documents — every element a LateChunkText, the
    elements of each document that document's chunks in order — and None for anything else (a mixed list, a
    re-ordered or partial one, plain strings)."""
    out, i, n = [], 0, len(texts)
    if n == 0:
        return None
    while i < n:
        first = texts[i]
        if type(first) is not LateChunkText or first.late_index != 0:
            return None
        doc = first.late_doc
        if i + doc.n_chunks > n:
            return None
        for k in range(doc.n_chunks):
            t = texts[i + k]
            if type(t) is not LateChunkText or t.late_doc is not doc or t.late_index != k:
                return None
        out.append((doc.text, [str(t) for t in texts[i:i + doc.n_chunks]]))
        i += doc.n_chunks
    return out
