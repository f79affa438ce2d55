"""Late chunking without a GPU (voitta_rag_amd/late_chunking.py): how a document and its chunks become
token sequences and token spans — location, segments, spans, windows, the passage prefix — then the two settings, the
``LateChunkText`` the drop-in chunker hands out, and the route ``embed_texts`` takes for it.

The chunks come from the reference chunker's restatement (voitta_rag_amd.chunking). The first tokenizer is a stub with
one id per whitespace-separated word, so that expected spans can be written by hand; the second pass uses the native
WordPiece on a small vocabulary."""
import numpy as np
import pytest

from voitta_rag_amd import late_chunking as lc

CLS, SEP = 1, 2


class WordStub:
    """One id per whitespace-separated word (ids from 10 on, in order of first appearance), [CLS] ... [SEP] around every
    text, packed the way NativeSentenceEncoder.tokenize packs."""

    def __init__(self):
        self.vocab = {}

    def words(self, text):
        return [self.vocab.setdefault(w, 10 + len(self.vocab)) for w in text.split()]

    def __call__(self, texts):
        ids, off = [], [0]
        for t in texts:
            ids += [CLS] + self.words(t) + [SEP]
            off.append(len(ids))
        return np.asarray(ids, np.int32), np.asarray(off, np.int32)


PARAGRAPHS = [
    "Late chunking embeds every chunk in the context of its whole document. The document goes through the encoder once.",
    "Each chunk's vector is then the mean of the final hidden states of that chunk's own tokens! Nothing else changes?",
    "The default was 16 until version 2.3. It was raised to 32 in the next release, and nobody remembered why.",
    "A short one.",
    "Sentences without a full stop at the end of a paragraph also occur\nas do single newlines inside a paragraph",
]
DOCUMENT = "\n\n".join(PARAGRAPHS) + "\n"
LONG = "\n\n".join(f"Paragraph {i} talks about item{i} and item{i + 1}. It has a second sentence about thing{i}."
                   for i in range(30))


def documents_for(strategy):
    """The sentence strategy joins sentences with one space whatever separated them (chunking.py:209-214), so its chunks
    are pieces of the document only where one space did: it is run on the same texts with single spaces. (On the
    originals its chunks are not found, and the document goes the plain way: see the test of that below.)"""
    if strategy == "sentence":
        return [" ".join(DOCUMENT.split()), " ".join(LONG.split())]
    return [DOCUMENT, LONG]


def chunks_of(text, strategy, overlap, size=120):
    from voitta_rag_amd.chunking import ChunkingService

    cs = ChunkingService(size, 50, strategy)
    cs.chunk_overlap = overlap  # (the constructor reads 0 as "use the setting", as the reference's does)
    return [c.text for c in cs.chunk_text(text)]


def segments_of(document, where):
    cuts = sorted({0, len(document)} | {p for se in where for p in se})
    return cuts, [document[a:b] for a, b in zip(cuts, cuts[1:])]


def inside_word(document, p, is_word_char):
    return 0 < p < len(document) and is_word_char(document[p - 1]) and is_word_char(document[p])


def check_plan(document, chunk_texts, tokenize, is_word_char, prefix=()):
    """The properties every one-window plan has; returns the plan."""
    where = lc.locate(document, chunk_texts)
    assert where is not None and len(where) == len(chunk_texts)
    starts = [s for s, _ in where]
    assert starts == sorted(starts)
    for (s, e), text in zip(where, chunk_texts):
        assert document[s:e].strip() == text and text
    p = lc.plan(document, chunk_texts, tokenize, 8192, 256, prefix)
    assert p is not None and p.n_seq == 1 and p.n_chunks == len(chunk_texts) and not p.truncated.any()
    assert p.span_off.tolist() == [0, len(chunk_texts)] and p.offsets.tolist() == [0, len(p.ids)]
    shift = 1 + len(prefix)
    assert p.ids[0] == CLS and p.ids[-1] == SEP and p.ids[1:shift].tolist() == list(prefix)
    body = p.ids[shift:-1]
    # the concatenated segment tokens are the sequence minus specials and prefix
    cuts, segs = segments_of(document, where)
    pieces, _ = lc.strip_specials(*tokenize([s for s in segs if s.strip()]))
    assert np.array_equal(np.concatenate(pieces), body)
    # a chunk's span holds the chunk tokenised alone, unless a cut (its own ends, or another chunk's boundary inside
    # it) falls inside a word: that word is then tokenised as two pieces
    compared = 0
    for (s, e), text, (b, en) in zip(where, chunk_texts, p.span_tok.tolist()):
        assert shift <= b < en <= len(p.ids) - 1
        if any(inside_word(document, c, is_word_char) for c in cuts if s <= c <= e):
            continue
        alone, _ = lc.strip_specials(*tokenize([text]))
        assert np.array_equal(p.ids[b:en], alone[0]), text
        compared += 1
    return p, compared


# ---- location, segments, spans ---------------------------------------------------------------------------------------------
def test_a_hand_written_plan():
    tok = WordStub()
    p = lc.plan("a b c d e  f", ["a b c", "c d e", "f"], tok, 32, 8)
    a, b, c, d, e, f = (tok.vocab[w] for w in "abcdef")
    assert p.ids.tolist() == [CLS, a, b, c, d, e, f, SEP] and p.offsets.tolist() == [0, 8]
    assert p.span_off.tolist() == [0, 3] and p.span_tok.tolist() == [[1, 4], [3, 6], [6, 7]]
    assert not p.truncated.any() and p.ids.dtype == p.offsets.dtype == p.span_off.dtype == p.span_tok.dtype == np.int32
    # a cut inside a word: "de" is tokenised as "d" and "e", the chunks' own texts start / end with those fragments
    tok = WordStub()
    p = lc.plan("ab cd ef", ["ab c", "d ef"], tok, 32, 8)
    assert p.ids.tolist() == [CLS] + [tok.vocab[w] for w in ("ab", "c", "d", "ef")] + [SEP]
    assert p.span_tok.tolist() == [[1, 3], [3, 5]]


@pytest.mark.parametrize("overlap", [0, 50])
@pytest.mark.parametrize("strategy", ["recursive", "sentence", "fixed"])
def test_chunker_output_is_located_and_spanned_with_the_word_stub(strategy, overlap):
    compared = 0
    for document in documents_for(strategy):
        chunks = chunks_of(document, strategy, overlap)
        assert len(chunks) >= 4
        _, n = check_plan(document, chunks, WordStub(), lambda ch: not ch.isspace())
        compared += n
    assert compared >= 2
    if overlap == 0 and strategy != "fixed":  # nothing cut inside a word: the sequence is the document's own tokens
        tok = WordStub()
        long = documents_for(strategy)[1]
        p = lc.plan(long, chunks_of(long, strategy, 0), tok, 8192, 256)
        assert p.ids[1:-1].tolist() == tok.words(long)


def test_sentence_chunks_across_paragraph_breaks_send_the_document_the_plain_way():
    """The sentence strategy re-joins sentences with one space: across a blank line such a chunk is no piece of the
    document, plan gives None, and the caller encodes that document's chunks the plain way."""
    chunks = chunks_of(DOCUMENT, "sentence", 0)
    assert any(c not in DOCUMENT for c in chunks) and lc.locate(DOCUMENT, chunks) is None
    assert lc.plan(DOCUMENT, chunks, WordStub(), 8192, 256) is None


def test_overlap_tails_cut_words_at_this_chunk_size():
    """The case the parametrised test must contain: with overlap 50 at 120 characters some chunk starts inside a word."""
    chunks = chunks_of(LONG, "recursive", 50)
    where = lc.locate(LONG, chunks)
    assert any(inside_word(LONG, s, lambda ch: not ch.isspace()) for s, _ in where)


@pytest.mark.parametrize("overlap", [0, 50])
@pytest.mark.parametrize("strategy", ["recursive", "sentence", "fixed"])
def test_chunker_output_with_the_native_wordpiece(strategy, overlap):
    from voitta_rag_amd.wordpiece import WordPieceTokenizer

    words = sorted({w.strip(".,!?'").lower() for w in (DOCUMENT + " " + LONG).split()} - {""})
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", ".", ",", "!", "?", "'"] + words[::2] + \
        ["##" + ch for ch in "abcdefghijklmnopqrstuvwxyz0123456789"] + list("abcdefghijklmnopqrstuvwxyz0123456789")
    wp = WordPieceTokenizer(vocab, max_length=8192)
    cls, sep = vocab.index("[CLS]"), vocab.index("[SEP]")

    def tokenize(texts):
        ids, off = wp.encode_batch(list(texts))
        ids = ids.copy()
        ids[off[:-1]], ids[off[1:] - 1] = CLS, SEP  # (the checks above know the specials as CLS, SEP)
        return ids, off.astype(np.int32)

    assert (cls, sep) == (2, 3)
    compared = 0
    for document in documents_for(strategy):
        _, n = check_plan(document, chunks_of(document, strategy, overlap), tokenize, str.isalnum, prefix=(40, 41))
        compared += n
    assert compared >= 2


def test_a_repeated_paragraph_is_located_at_its_second_occurrence():
    rep = "The same paragraph again."
    document = f"{rep}\n\nSomething else in between here.\n\n{rep}\n\nThe end."
    chunks = [rep, "Something else in between here.", rep, "The end."]
    where = lc.locate(document, chunks)
    second = document.index(rep, 1)
    assert where[0] == (0, len(rep)) and where[2] == (second, second + len(rep)) and second > where[1][0]
    tok = WordStub()
    p = lc.plan(document, chunks, tok, 64, 8)
    assert p.span_tok.tolist() == [[1, 5], [5, 10], [10, 14], [14, 16]]
    # two chunks with one text, the second starting where the first does: both found (at or after, not after)
    assert lc.locate("x y x y", ["x y", "x y"]) == [(0, 3), (0, 3)]


def test_a_chunk_that_is_not_in_the_document_gives_none():
    tok = WordStub()
    assert lc.plan("alpha beta gamma", ["alpha beta", "delta"], tok, 32, 8) is None
    assert lc.plan("alpha beta gamma", ["gamma", "alpha"], tok, 32, 8) is None  # out of document order
    assert lc.plan("alpha beta gamma", ["alpha", ""], tok, 32, 8) is None
    assert lc.plan("alpha beta", [], tok, 32, 8) is None
    # ... and plan_many sends such a document the plain way inside the same result
    p = lc.plan_many([("alpha beta gamma", ["alpha beta", "gamma"]), ("one two", ["one", "three four five"]), ("", [])],
                     tok, 32, 8, plain_text=lambda t: "p " + t)
    assert p.late == [True, False] and p.n_seq == 3 and p.n_chunks == 4
    assert p.span_off.tolist() == [0, 2, 3, 4] and p.offsets.tolist() == [0, 5, 9, 15]
    assert p.span_tok.tolist() == [[1, 3], [3, 4], [0, 4], [0, 6]]  # plain: the whole sequence, specials and prefix included
    cls = lc.plan_many([("one two", ["one", "three four five"])], tok, 32, 8, pooling="cls")
    assert cls.span_tok.tolist() == [[0, 1], [0, 1]]


# ---- windows ---------------------------------------------------------------------------------------------------------------
def five_word_chunks(n_chunks, tail_words=0):
    words = [f"w{i}" for i in range(5 * n_chunks + tail_words)]
    return " ".join(words), [" ".join(words[5 * j:5 * j + 5]) for j in range(n_chunks)]


def test_windows_by_hand():
    """32 tokens, context 8: L = 30. Chunk j holds tokens [5j, 5j + 5). The first window takes chunks 0..5 (30 tokens);
    a follow-on window starts 8 tokens before its first chunk and takes chunks while their end stays within 30 tokens of
    that start: 4 chunks (8 + 20 <= 30 < 8 + 25)."""
    document, chunks = five_word_chunks(20, tail_words=2)
    tok = WordStub()
    p = lc.plan(document, chunks, tok, 32, 8)
    assert p.span_off.tolist() == [0, 6, 10, 14, 18, 20]
    assert np.diff(p.offsets).tolist() == [32, 30, 30, 30, 8 + 10 + 2 + 2]  # the last one takes the 2 trailing tokens
    assert p.span_tok[:6].tolist() == [[1 + 5 * j, 6 + 5 * j] for j in range(6)]
    for first in (6, 10, 14, 18):
        assert p.span_tok[first].tolist() == [1 + 8, 1 + 13]
    ids = tok.words(document)
    assert p.ids[p.offsets[1] + 1:p.offsets[2] - 1].tolist() == ids[22:50]
    assert p.ids[p.offsets[4] + 1:p.offsets[5] - 1].tolist() == ids[82:102]
    assert not p.truncated.any()
    # a document of at most L tokens is one sequence, trailing tokens and all
    document, chunks = five_word_chunks(5, tail_words=5)
    p = lc.plan(document, chunks, WordStub(), 32, 8)
    assert p.offsets.tolist() == [0, 32] and p.span_off.tolist() == [0, 5]


@pytest.mark.parametrize("overlap", [0, 50])
def test_window_bounds_on_chunker_output(overlap):
    tok = WordStub()
    chunks = chunks_of(LONG, "recursive", overlap)
    p = lc.plan(LONG, chunks, tok, 32, 8)
    assert p.n_seq > 3 and p.n_chunks == len(chunks)
    assert np.diff(p.offsets).max() <= 32 and np.diff(p.offsets).min() >= 3
    # every chunk lies in exactly one window: span_off is a partition of the chunk list, in order, no window empty
    assert p.span_off[0] == 0 and p.span_off[-1] == len(chunks) and np.all(np.diff(p.span_off) >= 1)
    # absolute token positions of the chunks, worked out here from the located characters
    where = lc.locate(LONG, chunks)
    cuts, segs = segments_of(LONG, where)
    n_tok = np.cumsum([0] + [len(s.split()) for s in segs])
    cb = [int(n_tok[cuts.index(s)]) for s, _ in where]
    ce = [int(n_tok[cuts.index(e)]) for _, e in where]
    body = np.concatenate(lc.strip_specials(*tok([s for s in segs if s.strip()]))[0])
    for w in range(p.n_seq):
        first, last = int(p.span_off[w]), int(p.span_off[w + 1])
        seq = p.ids[p.offsets[w]:p.offsets[w + 1]]
        assert seq[0] == CLS and seq[-1] == SEP
        begin = int(p.span_tok[first, 0]) - 1
        # each window starts min(8, tokens available) before its first chunk: available in the document, and in the
        # window beside that chunk (one longer than L - context = 22 tokens gets the left context that still fits)
        assert begin == min(8, cb[first], max(0, 30 - (ce[first] - cb[first]))), (w, begin)
        ws = cb[first] - begin
        assert np.array_equal(seq[1:-1], body[ws:ws + len(seq) - 2])
        for c in range(first, last):
            assert p.span_tok[c].tolist() == [cb[c] - ws + 1, ce[c] - ws + 1] and ce[c] - ws <= 30
    assert not p.truncated.any()


def test_an_over_long_chunk_is_truncated_and_flagged():
    words = [f"w{i}" for i in range(100)]
    document = " ".join(words)
    # chunk 1: 25 tokens, more than L - context = 22: 5 tokens of left context still fit. chunk 2: 40 tokens, more than L.
    chunks = [" ".join(words[0:10]), " ".join(words[10:35]), " ".join(words[35:75]), " ".join(words[75:80])]
    tok = WordStub()
    p = lc.plan(document, chunks, tok, 32, 8)
    ids = tok.words(document)
    assert p.truncated.tolist() == [False, False, True, False]
    assert p.span_off.tolist() == [0, 1, 2, 3, 4]
    assert p.span_tok.tolist() == [[1, 11], [6, 31], [1, 31], [9, 14]]
    assert np.diff(p.offsets).tolist() == [12, 32, 32, 32]  # (the last: 8 of context, 5 of its own, 17 of the 20 trailing)
    assert p.ids[p.offsets[1] + 1:p.offsets[2] - 1].tolist() == ids[5:35]
    assert p.ids[p.offsets[2] + 1:p.offsets[3] - 1].tolist() == ids[35:65]
    assert p.ids[p.offsets[3] + 1:p.offsets[4] - 1].tolist() == ids[67:97]


def test_prefix_ids_shift_spans_and_count_against_the_window():
    document, chunks = five_word_chunks(12)
    tok = WordStub()
    prefix = (7, 8, 9)
    p = lc.plan(document, chunks, tok, 32, 8, prefix)  # L = 27: 5 chunks first, then 8 + 15 <= 27 < 8 + 20: 3 per window
    assert p.span_off.tolist() == [0, 5, 8, 11, 12] and np.diff(p.offsets).max() <= 32
    for w in range(p.n_seq):
        seq = p.ids[p.offsets[w]:p.offsets[w + 1]]
        assert seq[:4].tolist() == [CLS, 7, 8, 9] and seq[-1] == SEP
    assert p.span_tok[0].tolist() == [4, 9] and p.span_tok[5].tolist() == [4 + 8, 4 + 13] and p.span_tok.min() >= 4
    assert lc.prefix_ids_of("passage: ", tok) == (tok.vocab["passage:"],) and lc.prefix_ids_of("", tok) == ()
    with pytest.raises(ValueError, match="no room"):
        lc.plan(document, chunks, tok, 5, 0, prefix)


def test_plan_many_keeps_chunk_order_across_documents():
    tok = WordStub()
    d1, c1 = five_word_chunks(8)
    d2, c2 = "x1 x2 x3 x4", ["x1 x2", "x3 x4"]
    p1, p2 = lc.plan(d1, c1, WordStub(), 32, 8), lc.plan(d2, c2, WordStub(), 32, 8)
    p = lc.plan_many([(d1, c1), (d2, c2)], tok, 32, 8)
    assert p.n_seq == p1.n_seq + 1 and p.n_chunks == 10 and p.late == [True, True]
    assert p.span_off.tolist() == p1.span_off.tolist() + [10]
    assert p.offsets.tolist() == p1.offsets.tolist() + [int(p1.offsets[-1]) + 6]
    assert p.span_tok.tolist() == p1.span_tok.tolist() + p2.span_tok.tolist()
    n_seq, span_off, span_tok = p.spans()
    assert n_seq == p.n_seq and span_off is p.span_off and span_tok is p.span_tok
    empty = lc.plan_many([], tok, 32, 8)
    assert empty.n_seq == 0 and empty.n_chunks == 0 and empty.offsets.tolist() == [0]


# ---- settings --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def env(monkeypatch):
    from voitta_rag_amd import config

    def set_env(**values):
        for name, value in values.items():
            if value is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(value))
        config.get_settings.cache_clear()
        return config.get_settings()

    yield set_env
    for name in ("VOITTA_LATE_CHUNKING", "VOITTA_LATE_CHUNKING_CONTEXT", "VOITTA_MAX_SEQ_LENGTH", "VOITTA_DEFERRED_INDEXING"):
        monkeypatch.delenv(name, raising=False)
    config.get_settings.cache_clear()


def test_settings_defaults_and_ranges(env):
    s = env(VOITTA_LATE_CHUNKING=None, VOITTA_LATE_CHUNKING_CONTEXT=None, VOITTA_MAX_SEQ_LENGTH=None)
    assert s.late_chunking is False and s.late_chunking_context == 256
    assert env(VOITTA_LATE_CHUNKING=1).late_chunking is True
    assert env(VOITTA_LATE_CHUNKING=0).late_chunking is False
    for bad in ("2", "yes", "-1"):
        with pytest.raises(ValueError, match="VOITTA_LATE_CHUNKING"):
            env(VOITTA_LATE_CHUNKING=bad)
    env(VOITTA_LATE_CHUNKING=1)
    assert env(VOITTA_LATE_CHUNKING_CONTEXT=0).late_chunking_context == 0
    assert env(VOITTA_LATE_CHUNKING_CONTEXT=256).late_chunking_context == 256  # 512 / 2
    for bad in ("-1", "257"):
        with pytest.raises(ValueError, match="VOITTA_LATE_CHUNKING_CONTEXT"):
            env(VOITTA_LATE_CHUNKING_CONTEXT=bad)
    assert env(VOITTA_MAX_SEQ_LENGTH=8192, VOITTA_LATE_CHUNKING_CONTEXT=4096).late_chunking_context == 4096
    with pytest.raises(ValueError, match="VOITTA_LATE_CHUNKING_CONTEXT"):
        env(VOITTA_LATE_CHUNKING_CONTEXT=4097)
    # a cap below 512 with the context unset: the default follows the cap, nothing is refused
    assert env(VOITTA_MAX_SEQ_LENGTH=100, VOITTA_LATE_CHUNKING_CONTEXT=None).late_chunking_context == 50


def test_the_chunker_hands_out_plain_str_unless_the_setting_is_on(env):
    from voitta_rag_amd.chunking import ChunkingService

    env(VOITTA_LATE_CHUNKING=None)
    for c in ChunkingService(120, 50, "recursive").chunk_text(DOCUMENT):
        assert type(c.text) is str
    env(VOITTA_LATE_CHUNKING=1)
    docs = ChunkingService(120, 50, "recursive").chunk_texts([DOCUMENT, "", LONG])
    assert docs[1] == [] and len(docs[0]) >= 4
    for document, chunks in ((DOCUMENT, docs[0]), (LONG, docs[2])):
        for i, c in enumerate(chunks):
            assert type(c.text) is lc.LateChunkText and c.text.late_index == i == c.index
            assert c.text.late_doc is chunks[0].text.late_doc and c.text.late_doc.text == document
            assert c.text.late_doc.n_chunks == len(chunks)
    env(VOITTA_LATE_CHUNKING=None)
    plain = ChunkingService(120, 50, "recursive").chunk_texts([DOCUMENT, "", LONG])
    assert [[(c.text, c.index, c.start_char, c.end_char) for c in d] for d in plain] == \
        [[(str(c.text), c.index, c.start_char, c.end_char) for c in d] for d in docs]


def test_late_chunk_text_behaves_as_its_str():
    import copy
    import json
    import pickle

    doc = lc.LateDocument("Hello world, hello", 2)
    t = lc.LateChunkText("Hello world", doc, 0)
    s = "Hello world"
    assert t == s and s == t and not (t != s) and hash(t) == hash(s) and {t: 1}[s] == 1 and t in {s}
    assert t < "Hello x" and sorted([t, "A"]) == ["A", s] and len(t) == 11 and bool(t)
    assert t[:5] == "Hello" and type(t[:5]) is str and type(t + "!") is str and type(t.lower()) is str
    assert t.encode("utf-8") == s.encode("utf-8") and f"{t}" == s and f"passage: {t}" == "passage: " + s
    assert "%s|%5.3s" % (t, t) == "%s|%5.3s" % (s, s) and "{:>12}".format(t) == "{:>12}".format(s)
    assert str(t) == s and type(str(t)) is str and repr(t) == repr(s) and json.dumps(t) == json.dumps(s)
    assert t.split() == s.split() and t.startswith("Hello") and "world" in t and isinstance(t, str)
    for clone in (pickle.loads(pickle.dumps(t)), copy.deepcopy(t)):
        assert clone == s and type(clone) is str
    assert t.late_doc is doc and t.late_index == 0


# ---- routing ---------------------------------------------------------------------------------------------------------------
class FakeModel:
    """Records which entry point embed_texts reached."""

    max_seq_length = 512

    def __init__(self):
        self.calls = []

    def encode(self, texts, **_):
        self.calls.append(("encode", list(texts)))
        return np.zeros((len(texts), 4), np.float32)

    def encode_documents(self, documents, prefix=""):
        self.calls.append(("encode_documents", [(d, list(c)) for d, c in documents], prefix))
        return np.ones((sum(len(c) for _, c in documents), 4), np.float32)


def service(name="some-model"):
    from voitta_rag_amd.embedding import EmbeddingService

    svc = EmbeddingService(name)
    svc._model = FakeModel()
    return svc


def test_embed_texts_takes_the_late_route_only_for_complete_ordered_documents(env):
    env(VOITTA_LATE_CHUNKING=1, VOITTA_DEFERRED_INDEXING=0)
    a = lc.wrap_chunks("doc a: one two three", ["doc a: one", "two", "three"])
    b = lc.wrap_chunks("doc b: four", ["doc b: four"])
    svc = service()
    out = svc.embed_texts(a + b)
    assert svc._model.calls == [("encode_documents", [("doc a: one two three", ["doc a: one", "two", "three"]),
                                                      ("doc b: four", ["doc b: four"])], "")]
    assert out == [[1.0] * 4] * 4 and type(out) is list and type(out[0][0]) is float
    assert all(type(t) is str for _, chunks in svc._model.calls[0][1] for t in chunks)
    # the e5 rule reaches the late route as a prefix, not as concatenated text
    svc = service("intfloat/e5-base-v2")
    svc.embed_texts(b)
    assert svc._model.calls == [("encode_documents", [("doc b: four", ["doc b: four"])], "passage: ")]
    # anything else goes the plain route unchanged
    for texts in (a + ["plain"],                    # a mixed list
                  [a[1], a[0], a[2]],               # re-ordered
                  a[:2],                            # a document's chunks, but not all of them
                  a[1:],
                  a + b[:0] + a[:1],                # a second, partial copy
                  [str(t) for t in a],              # plain strings
                  [a[0], b[0], a[1], a[2]]):        # interleaved documents
        svc = service()
        svc.embed_texts(texts)
        assert svc._model.calls == [("encode", [str(t) for t in texts])], texts
    assert lc.group_documents([]) is None
    assert service().embed_texts([]) == []


def test_with_the_setting_off_late_chunk_texts_go_the_plain_route(env):
    env(VOITTA_LATE_CHUNKING=None, VOITTA_DEFERRED_INDEXING=0)
    a = lc.wrap_chunks("one two", ["one", "two"])
    svc = service("intfloat/e5-base-v2")
    svc.embed_texts(a)
    assert svc._model.calls == [("encode", ["passage: one", "passage: two"])]


def test_payloads_store_plain_text():
    from voitta_rag_amd.vector_store import ChunkMetadata, VectorStoreService

    t = lc.wrap_chunks("one two", ["one", "two"])[1]
    meta = ChunkMetadata(file_path="f", folder_path="d", index_folder="i", file_name="f", chunk_index=1, total_chunks=2,
                         start_char=4, end_char=7, indexed_at="now")
    payload = VectorStoreService._payload_of(t, meta)
    assert payload["text"] == "two" and type(payload["text"]) is str


# ---- BulkIndexer's batches, the warning at load --------------------------------------------------------------------------
def test_bulk_indexer_cuts_late_batches_at_file_boundaries(env):
    """With the setting on a batch is files until batch_chunks is reached, never half a file, and carries the plan of
    exactly its files; texts, metadata and counts are those of the plain mode."""
    from voitta_rag_amd.chunking import ChunkingService
    from voitta_rag_amd.indexer import BulkIndexer, ParsedFile

    class Embedder:
        model_name = "some-model"

        def __init__(self):
            self.model = self
            self.tok = WordStub()

        def _passage(self, text):
            return text

        def tokenize(self, texts):
            return self.tok(texts)

        def plan_documents(self, documents, prefix=""):
            return lc.plan_many(documents, self.tok, 64, 8, lc.prefix_ids_of(prefix, self.tok))

    contents = [LONG, "", DOCUMENT, "tiny file.", LONG[:700], " \n ", DOCUMENT[:300]]
    files = [ParsedFile(c, f"f{i}.md", "", "", f"f{i}.md") for i, c in enumerate(contents)]

    def batches(late):
        env(VOITTA_LATE_CHUNKING=1 if late else None)
        bulk = BulkIndexer(chunker=ChunkingService(120, 50, "recursive"), embedder=Embedder(), vector_store=object(),
                           sparse=False, batch_chunks=10, files_per_cut=3)
        return list(bulk._batches(iter(files)))

    late, plain = batches(True), batches(False)
    assert all(b.spans is None for b in plain) and max(len(b.texts) for b in plain) == 10
    flat = lambda bs, what: [x for b in bs for x in getattr(b, what)]  # noqa: E731
    assert flat(late, "texts") == flat(plain, "texts") and all(type(t) is str for t in flat(late, "texts"))
    strip = lambda ms: [{k: v for k, v in vars(m).items() if k != "indexed_at"} for m in ms]  # noqa: E731
    assert strip(flat(late, "metadatas")) == strip(flat(plain, "metadatas"))
    counts = {}
    for b in late:
        counts.update(b.counts)
    assert counts == {k: v for b in plain for k, v in b.counts.items()} and counts["f1.md"] == counts["f5.md"] == 0
    per_file = [counts[f.file_path] for f in files if counts[f.file_path]]
    assert len(late) >= 3 and per_file[0] > 10  # the first file alone is more than a batch: it stays whole
    seen = 0
    for b in late:
        n_seq, span_off, span_tok = b.spans
        sizes, total = [], 0
        while total < len(b.texts):  # whole files, and no more of them than it takes to reach batch_chunks
            sizes.append(per_file[seen + len(sizes)])
            total += sizes[-1]
        assert total == len(b.texts) and (total - sizes[-1] < 10)
        seen += len(sizes)
        assert len(b.wp_off) == n_seq + 1 == len(span_off) and span_off[-1] == len(b.texts) == len(span_tok)
        assert int(np.diff(b.wp_off).max()) <= 64
    assert seen == len(per_file)


def test_a_cls_pooled_checkpoint_warns_once_at_load_when_the_setting_is_on(env, monkeypatch, caplog):
    import logging

    from voitta_rag_amd import embedding
    from voitta_rag_amd import encoder as enc

    class Tokenizer:
        def no_padding(self):
            pass

        def enable_truncation(self, max_length):
            pass

    monkeypatch.setattr(embedding._enc, "load_encoder", lambda engine, desc, state: None)

    def warnings_for(pooling):
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="voitta_rag_amd.embedding"):
            embedding.NativeSentenceEncoder(None, enc.BertDesc(1, 64, 2, 128, vocab=10, max_pos=64, pooling=pooling), {},
                                            Tokenizer(), 64)
        return [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]

    env(VOITTA_LATE_CHUNKING=1)
    w = warnings_for("cls")
    assert len(w) == 1 and "VOITTA_LATE_CHUNKING" in w[0] and "[CLS]" in w[0]
    assert warnings_for("mean") == []
    env(VOITTA_LATE_CHUNKING=None)
    assert warnings_for("cls") == []
