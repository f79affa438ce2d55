"""Semantic chunking without a GPU: the oracle's rule on hand-written distances, the margins of the GPU
tests' fixtures, the host planner, the settings and the ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import semantic_case as sc
import semantic_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule on hand-written distances ------------------------------------------------------------------------------------
def test_break_budget_is_the_integer_ceiling():
    assert [so.break_budget(g, 50) for g in (0, 1, 19, 20, 21, 40, 41, 2047)] == [0, 1, 1, 1, 2, 2, 3, 103]
    assert [so.break_budget(20, p) for p in (0, 1, 49, 50, 51, 999, 1000)] == [0, 1, 1, 1, 2, 20, 20]


@pytest.mark.parametrize("gaps", [1, 19, 20, 21])
def test_the_largest_gaps_are_the_candidates_at_50_permille(gaps):
    rng = np.random.default_rng(gaps)
    d = rng.permutation(gaps).astype(np.float32) / 64.0
    cand = so.candidates(d, so.Params(break_permille=50))
    B = 2 if gaps == 21 else 1
    assert int(cand.sum()) == B and set(np.flatnonzero(cand)) == set(np.argsort(-d)[:B])


def test_ties_go_to_the_lowest_index():
    d = np.asarray([0.5, 0.75, 0.5, 0.75, 0.75, 0.25], np.float32)
    assert so.ranks(d).tolist() == [3, 0, 4, 1, 2, 5]
    assert so.candidates(d, so.Params(break_permille=300)).tolist() == [False, True, False, True, False, False]  # B = 2
    assert so.candidates(d, so.Params(break_permille=500)).tolist() == [False, True, False, True, True, False]
    ones = np.ones(20, np.float32)
    assert np.flatnonzero(so.candidates(ones, so.Params(break_permille=200))).tolist() == [0, 1, 2, 3]
    # the floor: a gap inside the budget but under min_distance is no candidate, and nobody takes its place
    assert so.candidates(d, so.Params(break_permille=1000, min_distance=0.5)).tolist() == [True] * 5 + [False]
    assert so.candidates(d, so.Params(break_permille=500, min_distance=0.8)).tolist() == [False] * 6
    assert not so.candidates(d, so.Params(break_permille=1000, min_distance=3.0)).any()


def test_min_and_max_tokens_in_the_walk():
    n = [10, 10, 10, 10, 10, 10]
    every = np.ones(5, bool)
    none = np.zeros(5, bool)
    assert so.walk(every, n, so.Params(min_tokens=0)).tolist() == [1, 1, 1, 1, 1, 1]
    assert so.walk(every, n, so.Params(min_tokens=20)).tolist() == [1, 0, 1, 0, 1, 0]   # a candidate waits for min_tokens
    assert so.walk(every, n, so.Params(min_tokens=25)).tolist() == [1, 0, 0, 1, 0, 0]
    assert so.walk(none, n, so.Params(max_tokens=30)).tolist() == [1, 0, 0, 1, 0, 0]    # max_tokens closes without one
    assert so.walk(none, n, so.Params(max_tokens=29)).tolist() == [1, 0, 1, 0, 1, 0]
    assert so.walk(none, n, so.Params()).tolist() == [1, 0, 0, 0, 0, 0]
    # max_tokens wins over min_tokens; the last chunk may stay under min_tokens
    one = np.asarray([0, 0, 0, 0, 1], bool)
    assert so.walk(one, n, so.Params(min_tokens=25, max_tokens=40)).tolist() == [1, 0, 0, 0, 1, 0]
    assert so.walk(one, [10, 10, 10, 10, 10, 3], so.Params(min_tokens=5, max_tokens=100)).tolist() == [1, 0, 0, 0, 0, 1]


def test_an_oversized_unit_is_a_chunk_of_its_own():
    n = [5, 50, 5, 5]
    assert so.walk(np.zeros(3, bool), n, so.Params(max_tokens=20)).tolist() == [1, 1, 1, 0]
    assert so.walk(np.zeros(2, bool), [50, 5, 5], so.Params(max_tokens=20)).tolist() == [1, 1, 0]
    assert so.walk(np.zeros(1, bool), [5, 50], so.Params(max_tokens=20)).tolist() == [1, 1]


def test_distances_and_chunk_means_of_a_hand_made_sequence():
    h = np.zeros((7, 4))
    h[0:2, 0] = 1.0   # unit 0: e0
    h[2:3, 0] = 3.0   # unit 1: e0
    h[4:7, 1] = 2.0   # unit 2: e1 (token 3 belongs to no unit)
    units = [(0, 2), (2, 3), (4, 7)]
    p = so.Params(buffer=0, break_permille=500)
    d, start, means = so.sequence(h, units, p)
    assert np.allclose(d, [0.0, 1.0]) and start.tolist() == [1, 0, 1]
    assert np.allclose(means, [[5.0 / 3.0, 0, 0, 0], [0, 2.0, 0, 0]])
    d1 = so.distances(so.unit_sums(h, units), 1)  # C_0 = S_0 + S_1, C_1 = all three, C_2 = S_1 + S_2
    assert np.allclose(d1, [1 - 5 / np.sqrt(61), 1 - 51 / np.sqrt(61 * 45)])
    assert np.allclose(so.distances(so.unit_sums(h, units), 3), [0.0, 0.0])  # every C_r the sum of all units
    assert so.sequence(h, [], p)[1].shape == (0,) and so.sequence(h, units[:1], p)[1].tolist() == [1]


def test_replay_compares_f32_as_stored():
    a = np.float32(0.3)
    d = np.asarray([a, np.nextafter(a, np.float32(1)), a, 0.0], np.float32)  # (the last of the sequence: unused)
    tok = np.asarray([(0, 1), (1, 2), (2, 3), (3, 4)], np.int32)
    assert so.replay(d, [0, 4], tok, so.Params(break_permille=300)).tolist() == [1, 0, 1, 0]  # B = 1: the one ulp decides
    assert so.replay(d, [0, 4], tok, so.Params(break_permille=300, min_distance=float(a))).tolist() == [1, 0, 1, 0]
    assert so.replay(d, [0, 0, 4], tok, so.Params(break_permille=1000)).tolist() == [1, 1, 1, 1]


# ---- the fixtures of test_semantic_gpu.py ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.BY_NAME))
def test_fixture_margins_are_more_than_twice_the_distance_bound(name):
    """Both margins — between the B-th and the (B + 1)-th distance, and from min_distance — of every sequence, at every
    precision the fixture is held against the oracle at."""
    fx = sc.BY_NAME[name]
    assert fx.precisions
    for precision in fx.precisions:
        need = 2.0 * sc.distance_bound(fx.model.hidden_size, precision)
        for d, start, _ in fx.oracle():
            rank_margin, floor_margin = so.margins(d, fx.params)
            assert rank_margin > need and floor_margin > need, (name, precision, rank_margin, floor_margin, need)
            assert 1 < int(start.sum()) < len(start)


def test_the_bound_is_two_root_h_tol():
    from test_encoder_gpu import TOL

    assert sc.distance_bound(128, "f32") == pytest.approx(2 * np.sqrt(128) * 2e-5) and TOL["f16"][1] == 5e-4
    assert sc.distance_bound(1024, "f16") == pytest.approx(0.032)


# ---- the planner -------------------------------------------------------------------------------------------------------------
def word_tokenize(texts):
    """[CLS]=1 word ids [SEP]=2: one id per whitespace-separated word."""
    ids, off = [], [0]
    for t in texts:
        ids += [1] + [3 + (sum(map(ord, w)) % 97) for w in t.split()] + [2]
        off.append(len(ids))
    return np.asarray(ids, np.int32), np.asarray(off, np.int32)


def _sentences(n, seed=0):
    rng = np.random.default_rng(seed)
    words = ["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta", "theta"]
    return [" ".join(rng.choice(words, size=int(rng.integers(4, 9)))).capitalize() + "." for _ in range(n)]


def test_units_to_chunks_to_texts_round_trip():
    from voitta_rag_amd import semantic_chunking as sem

    sents = _sentences(12, 1)
    doc = "  " + " ".join(sents[:5]) + "\n\n" + "  ".join(sents[5:]) + " \n"
    up = sem.plan_units([(doc, sents), ("", []), ("Other text. More text.", ["Other text.", "More text."])], word_tokenize, 512, 64)
    assert up.planned == [0, 2] and up.plain == [1] and up.plan.n_seq == 2 and up.plan.span_off.tolist() == [0, 12, 14]
    where = up.where[0]
    assert [doc[a:b] for a, b in where] == sents
    tok = up.plan.span_tok[:12]
    assert tok[0, 0] == 1 and np.array_equal(tok[1:, 0], tok[:-1, 1])  # [CLS] is nobody's; the units tile the words
    start = [1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0]
    chunks = sem.rebuild(doc, where, start)
    assert [c[0] for c in chunks] == [doc[where[a][0]:where[b][1]] for a, b in ((0, 2), (3, 4), (5, 9), (10, 11))]
    assert all(doc[a:b] == t for t, a, b in chunks)
    assert chunks[0][0] == " ".join(sents[:3]) and chunks[1][0] == " ".join(sents[3:5])
    assert chunks[2][0] == "  ".join(sents[5:10])  # (what lies between two units of a chunk belongs to its text)
    words = [w for t, _, _ in chunks for w in t.split()]
    assert words == doc.split()  # nothing lost, nothing twice
    with pytest.raises(ValueError):
        sem.rebuild(doc, where, [0] + start[1:])
    assert sem.rebuild("", [], []) == []


def test_units_of_the_sentence_strategy_are_found_across_paragraph_breaks():
    """The native `sentence` strategy packs sentences into a unit with one space between them, whatever separated them
    in the document: the planner finds such a unit by its words and plans its verbatim slice."""
    from voitta_rag_amd import semantic_chunking as sem
    from voitta_rag_amd.chunking import ChunkingService

    sents = _sentences(9, 5)
    doc = sents[0] + "  " + sents[1] + "\n\n" + " ".join(sents[2:5]) + "\n\n\n" + "\t".join(sents[5:]) + "\n"
    splitter = ChunkingService(chunk_size=100, strategy="sentence")
    splitter.chunk_overlap = 0
    units = [str(c.text) for c in splitter.cut([doc])[0]]
    assert len(units) > 3 and any(u not in doc for u in units)  # (the case: a unit that is no substring)
    anchored = sem.anchor_units(doc, units)
    assert [a.split() for a in anchored] == [u.split() for u in units] and all(a in doc for a in anchored)
    up = sem.plan_units([(doc, units)], word_tokenize, 512, 64)
    assert up.planned == [0] and [doc[a:b] for a, b in up.where[0]] == anchored
    assert all(a[1] <= b[0] for a, b in zip(up.where[0], up.where[0][1:]))
    n_words = int(up.plan.span_tok[-1, 1]) - 1
    assert n_words == len(doc.split()) and np.array_equal(up.plan.span_tok[1:, 0], up.plan.span_tok[:-1, 1])
    chunks = sem.rebuild(doc, up.where[0], [1] + [0] * (len(units) - 1))
    assert chunks == [(doc.strip(), 0, len(doc.strip()))]
    assert sem.anchor_units(doc, units[:1] + ["Nowhere to be found."]) is None and sem.anchor_units(doc, [" "]) is None


def test_windows_never_share_a_chunk():
    """A document of 40 units in windows of 64 tokens: every window is a sequence of its own, the first unit of a
    sequence starts a chunk whatever the distances say, and so no rebuilt chunk holds units of two windows."""
    from voitta_rag_amd import semantic_chunking as sem

    sents = _sentences(40, 2)
    doc = " ".join(sents)
    up = sem.plan_units([(doc, sents)], word_tokenize, 64, 16)
    p = up.plan
    assert p.n_seq > 3 and int(p.span_off[-1]) == 40 and np.all(np.diff(p.offsets) <= 64)
    params = so.Params(break_permille=0)  # no candidate at all: one chunk per window
    start = so.replay(np.zeros(40, np.float32), p.span_off, p.span_tok, params)
    assert np.flatnonzero(start).tolist() == p.span_off[:-1].tolist()
    chunks = sem.rebuild(doc, up.where[0], start)
    assert len(chunks) == p.n_seq
    for (text, a, b), lo, hi in zip(chunks, p.span_off[:-1], p.span_off[1:]):
        assert text == " ".join(sents[int(lo):int(hi)]) == doc[a:b]
    for i in range(p.n_seq):  # in order and never overlapping inside every window, as the engine demands
        tok = p.span_tok[int(p.span_off[i]):int(p.span_off[i + 1])]
        assert np.all(tok[:, 0] < tok[:, 1]) and np.all(tok[1:, 0] >= tok[:-1, 1])
        assert tok[-1, 1] <= p.offsets[i + 1] - p.offsets[i] - 1


def test_a_document_with_an_unlocatable_unit_goes_the_plain_way():
    from voitta_rag_amd import semantic_chunking as sem

    sents = _sentences(4, 3)
    doc = " ".join(sents)
    up = sem.plan_units([(doc, sents[:2] + ["Not in the text."] + sents[2:]), (doc, sents), (doc, ["   "])], word_tokenize, 512, 64)
    assert up.plain == [0, 2] and up.planned == [1] and int(up.plan.span_off[-1]) == 4
    # the same sentence twice in a row is located twice at one place: not in order, the plain way
    up = sem.plan_units([("Same. Same.", ["Same.", "Same."])], word_tokenize, 512, 64)
    assert up.plain == [0] and up.plan.n_chunks == 0


def test_chunk_texts_carry_their_vectors_as_plain_strings():
    import copy
    import pickle

    from voitta_rag_amd import semantic_chunking as sem

    va, vb = np.arange(6, dtype=np.float32).reshape(3, 2), np.ones((1, 2), np.float32)
    a, b = sem.wrap_chunks(["x", "y", "z"], va), sem.wrap_chunks(["x"], vb)
    assert a[0] == "x" and hash(a[1]) == hash("y") and type(a[0] + "") is str and type(a[0][:1]) is str
    assert type(pickle.loads(pickle.dumps(a[0]))) is str and type(copy.deepcopy(a[2])) is str
    assert np.array_equal(sem.carried_vectors(a + b), np.concatenate([va, vb]))
    assert np.array_equal(sem.carried_vectors(b + a), np.concatenate([vb, va]))
    for other in (a[:2], a[1:], [a[0], a[2], a[1]], a + ["x"], ["x", "y", "z"], [a[0], b[0], a[2]], []):
        assert sem.carried_vectors(other) is None


# ---- settings ----------------------------------------------------------------------------------------------------------------
SEMANTIC_ENV = ("VOITTA_SEMANTIC_CHUNKING", "VOITTA_SEMANTIC_UNIT_CHARS", "VOITTA_SEMANTIC_BUFFER",
                "VOITTA_SEMANTIC_BREAK_PERMILLE", "VOITTA_SEMANTIC_MIN_DISTANCE", "VOITTA_SEMANTIC_MIN_TOKENS",
                "VOITTA_SEMANTIC_MAX_TOKENS", "VOITTA_LATE_CHUNKING", "VOITTA_MAX_SEQ_LENGTH")


@pytest.fixture
def env(monkeypatch):
    for name in SEMANTIC_ENV:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def test_settings_defaults_and_values(env):
    from voitta_rag_amd.config import Settings

    s = Settings()
    assert not s.semantic_chunking and (s.semantic_buffer, s.semantic_break_permille, s.semantic_min_distance) == (1, 50, 0.0)
    assert (s.semantic_unit_chars, s.semantic_min_tokens, s.semantic_max_tokens) == (200, 32, 256)
    for name, value in (("CHUNKING", "1"), ("UNIT_CHARS", "120"), ("BUFFER", "3"), ("BREAK_PERMILLE", "100"),
                        ("MIN_DISTANCE", "0.25"), ("MIN_TOKENS", "8"), ("MAX_TOKENS", "64")):
        env.setenv("VOITTA_SEMANTIC_" + name, value)
    s = Settings()
    assert s.semantic_chunking and (s.semantic_unit_chars, s.semantic_buffer, s.semantic_break_permille) == (120, 3, 100)
    assert (s.semantic_min_distance, s.semantic_min_tokens, s.semantic_max_tokens) == (0.25, 8, 64)
    env.setenv("VOITTA_SEMANTIC_CHUNKING", " ")
    assert not Settings().semantic_chunking
    env.setenv("VOITTA_MAX_SEQ_LENGTH", "128")  # the defaults follow the window
    env.delenv("VOITTA_SEMANTIC_MAX_TOKENS")
    env.delenv("VOITTA_SEMANTIC_MIN_TOKENS")
    assert (Settings().semantic_min_tokens, Settings().semantic_max_tokens) == (32, 128)


@pytest.mark.parametrize("name,value,message", [
    ("VOITTA_SEMANTIC_CHUNKING", "yes", "VOITTA_SEMANTIC_CHUNKING=yes: accepted values are 0 and 1"),
    ("VOITTA_SEMANTIC_CHUNKING", "2", "VOITTA_SEMANTIC_CHUNKING=2: accepted values are 0 and 1"),
    ("VOITTA_SEMANTIC_UNIT_CHARS", "8", "VOITTA_SEMANTIC_UNIT_CHARS=8: accepted values are 16 ... 65536"),
    ("VOITTA_SEMANTIC_BUFFER", "4", "VOITTA_SEMANTIC_BUFFER=4: accepted values are 0 ... 3"),
    ("VOITTA_SEMANTIC_BUFFER", "one", "VOITTA_SEMANTIC_BUFFER=one: accepted values are 0 ... 3"),
    ("VOITTA_SEMANTIC_BREAK_PERMILLE", "1001", "VOITTA_SEMANTIC_BREAK_PERMILLE=1001: accepted values are 0 ... 1000"),
    ("VOITTA_SEMANTIC_BREAK_PERMILLE", "-1", "VOITTA_SEMANTIC_BREAK_PERMILLE=-1: accepted values are 0 ... 1000"),
    ("VOITTA_SEMANTIC_MIN_DISTANCE", "2.5", "VOITTA_SEMANTIC_MIN_DISTANCE=2.5: accepted values are 0 ... 2"),
    ("VOITTA_SEMANTIC_MIN_DISTANCE", "nan", "VOITTA_SEMANTIC_MIN_DISTANCE=nan: accepted values are 0 ... 2"),
    ("VOITTA_SEMANTIC_MIN_DISTANCE", "far", "VOITTA_SEMANTIC_MIN_DISTANCE=far: accepted values are 0 ... 2"),
    ("VOITTA_SEMANTIC_MAX_TOKENS", "0", "VOITTA_SEMANTIC_MAX_TOKENS=0: accepted values are 1 ... 512"),
    ("VOITTA_SEMANTIC_MAX_TOKENS", "513", r"VOITTA_SEMANTIC_MAX_TOKENS=513: accepted values are 1 ... 512 \(VOITTA_MAX_SEQ_LENGTH=512\)"),
    ("VOITTA_SEMANTIC_MIN_TOKENS", "257", r"VOITTA_SEMANTIC_MIN_TOKENS=257: accepted values are 0 ... 256 \(VOITTA_SEMANTIC_MAX_TOKENS=256\)"),
    ("VOITTA_SEMANTIC_MIN_TOKENS", "-1", "VOITTA_SEMANTIC_MIN_TOKENS=-1: accepted values are 0 ... 256"),
])
def test_bad_settings_are_refused(env, name, value, message):
    from voitta_rag_amd.config import Settings

    env.setenv(name, value)
    with pytest.raises(ValueError, match=message):
        Settings()


def test_semantic_and_late_chunking_together_are_refused_by_name(env):
    from voitta_rag_amd.config import Settings

    env.setenv("VOITTA_LATE_CHUNKING", "1")
    assert Settings().late_chunking and not Settings().semantic_chunking
    env.setenv("VOITTA_SEMANTIC_CHUNKING", "1")
    with pytest.raises(ValueError, match="VOITTA_SEMANTIC_CHUNKING=1 together with VOITTA_LATE_CHUNKING=1"):
        Settings()


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_semantic_params_layout_matches_the_header(tmp_path):
    from voitta_rag_amd import _lib

    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "voitta_engine.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu\\n",sizeof(vr_semantic_params),offsetof(vr_semantic_params,buffer),'
                   'offsetof(vr_semantic_params,max_tokens),offsetof(vr_semantic_params,min_distance));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _lib.VrSemanticParams
    assert sizes == [C.sizeof(S), S.buffer.offset, S.max_tokens.offset, S.min_distance.offset] == [24, 4, 16, 20]
    assert [f[0] for f in S._fields_] == ["struct_size", "buffer", "break_permille", "min_tokens", "max_tokens", "min_distance"]


def test_the_binding_matches_the_header_and_the_library():
    from voitta_rag_amd import _lib

    header = open(os.path.join(ROOT, "include", "voitta_engine.h")).read()
    proto = re.search(r"int vr_encode_semantic\((.*?)\);", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    args = [a.strip() for a in proto.split(",")]
    restype, argtypes = _lib.SIGNATURES["vr_encode_semantic"]
    assert restype is C.c_int and len(argtypes) == len(args) == 13
    for a, t in zip(args, argtypes):
        if "*" in a and "params" not in a and "n_chunks" not in a:
            assert t is C.c_void_p, a
        elif "*" not in a:
            assert t in (C.c_int, C.c_int32), a
    assert argtypes[7]._type_ is _lib.VrSemanticParams and argtypes[11]._type_ is C.c_int32
    assert hasattr(_lib.load_library(), "vr_encode_semantic")
    from voitta_rag_amd import Engine

    assert callable(Engine.encode_semantic)
