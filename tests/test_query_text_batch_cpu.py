"""No-GPU checks of vr_query_text_batch (n questions as text, each with its own filter, limit and sparse weight): the
library exports it, the ctypes table declares it with the header's argument types, n = 0 does nothing, and malformed
input is rejected with a message before the engine is touched (a NULL engine: valid input reaches the engine check,
bad input never does)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vr_query_text_batch"


def test_library_exports_the_call():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    assert hasattr(lib, NAME)
    assert NAME in _lib.SIGNATURES


def _header_params(name):
    src = open(os.path.join(ROOT, "include", "voitta_engine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
    assert m, name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def test_ctypes_declaration_follows_the_header():
    from voitta_rag_amd import _lib

    base = {"int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int, "float": C.c_float, "double": C.c_double,
            "vr_filter": _lib.VrFilter}
    params = _header_params(NAME)
    restype, argtypes = _lib.SIGNATURES[NAME]
    assert restype is C.c_int
    assert len(argtypes) == len(params) == 21, params
    for p, a in zip(params, argtypes):
        t = p.rsplit(" ", 1)[0].replace("const", "").replace("*", "").strip()
        stars = p.count("*")
        if t in ("vr_engine", "vr_wordpiece"):
            assert a is C.c_void_p, p
        elif t == "char":
            assert stars == 2 and a == C.POINTER(C.c_char_p), p
        else:
            assert a == (C.POINTER(base[t]) if stars else base[t]), (p, a)


def _last_error(lib):
    return lib.vr_last_error().decode()


def _call(lib, n=3, limits=None, foq=None, n_filters=2, out_stride=None, fusion=0, max_len=32, tokenizer=1,
          dense=None, dense_lens=None, sparse=None, sparse_lens=None, struct_size=None, must_sets=None):
    from voitta_rag_amd import SearchFilter, _lib

    farr = (_lib.VrFilter * max(n_filters, 1))()
    keep = []
    for j in range(max(n_filters, 1)):
        f, k = SearchFilter(exclude_folders=[j]).to_c()
        if struct_size is not None:
            f.struct_size = struct_size
        if must_sets is not None:
            f.n_must_folder_sets = must_sets
        farr[j] = f
        keep.append(k)
    texts = dense if dense is not None else [b"query: vector search"] * n
    d_arr = (C.c_char_p * max(n, 1))(*texts[:n])
    d_len = np.array(dense_lens if dense_lens is not None else [len(t or b"") for t in texts[:n]] or [0], np.int64)
    sp = sparse if sparse is not None else [b"vector search"] * n
    s_arr = (C.c_char_p * max(n, 1))(*sp[:n])
    s_len = np.array(sparse_lens if sparse_lens is not None else [len(t or b"") for t in sp[:n]] or [0], np.int64)
    lim = np.asarray(limits if limits is not None else [10] * n or [1], np.int32)
    w = np.full(max(n, 1), 0.1, np.float64)
    f = np.asarray(foq if foq is not None else [0, 1, -1, 0][:n] or [0], np.int32)
    stride = out_stride if out_stride is not None else max(1, int(lim.max()))
    rows = np.zeros((max(n, 1), stride), np.int64)
    scores = np.zeros((max(n, 1), stride), np.float64)
    fd = np.zeros((max(n, 1), stride), np.int32)
    counts = np.full(max(n, 1), -7, np.int32)
    hyb = np.full(max(n, 1), -7, np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    rc = lib.vr_query_text_batch(None, C.c_void_p(tokenizer) if tokenizer else None, n, d_arr, p(d_len, C.c_int64), s_arr,
                                 p(s_len, C.c_int64), max_len, p(lim, C.c_int32), p(w, C.c_double), fusion, farr,
                                 n_filters, p(f, C.c_int32), stride, p(rows, C.c_int64), p(scores, C.c_double),
                                 p(fd, C.c_int32), p(counts, C.c_int32), p(hyb, C.c_int32), None)
    del keep
    return rc, counts, hyb


def test_valid_input_reaches_the_engine_check():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    assert _call(lib)[0] != 0 and "null engine" in _last_error(lib)
    assert _call(lib, limits=[1, 100, 341], out_stride=341)[0] != 0 and "null engine" in _last_error(lib)
    assert _call(lib, sparse=[None, b"", b"x"], sparse_lens=[0, 0, 1])[0] != 0 and "null engine" in _last_error(lib)
    assert _call(lib, foq=[-1, -1, -1], n_filters=0)[0] != 0 and "null engine" in _last_error(lib)


def test_zero_questions_touch_nothing():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    rc, counts, hyb = _call(lib, n=0)
    assert rc == 0
    assert counts[0] == -7 and hyb[0] == -7


@pytest.mark.parametrize("foq", [[0, 2, 0], [-2, 0, 0], [0, 1, 1 << 30]])
def test_filter_of_query_out_of_range(foq):
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    assert _call(lib, foq=foq)[0] != 0 and "filter_of_query" in _last_error(lib)


def test_malformed_filters_are_rejected():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    assert _call(lib, struct_size=8)[0] != 0 and "size mismatch" in _last_error(lib)
    assert _call(lib, must_sets=3)[0] != 0 and "must-sets" in _last_error(lib)
    assert _call(lib, n_filters=-1)[0] != 0 and "bad filters" in _last_error(lib)


@pytest.mark.parametrize("bad", [0, -3, 342, 1 << 20])
def test_limits_are_checked(bad):
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    assert _call(lib, limits=[10, bad, 10], out_stride=400)[0] != 0
    assert "limits[1]" in _last_error(lib)


def test_other_arguments_are_checked():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    assert _call(lib, limits=[10, 20, 5], out_stride=19)[0] != 0 and "out_stride" in _last_error(lib)
    assert _call(lib, fusion=7)[0] != 0 and "unknown fusion 7" in _last_error(lib)
    assert _call(lib, max_len=1)[0] != 0 and "max_len 1" in _last_error(lib)
    assert _call(lib, max_len=5000)[0] != 0 and "max_len 5000" in _last_error(lib)
    assert _call(lib, n=-1)[0] != 0 and "bad arguments" in _last_error(lib)
    assert _call(lib, tokenizer=0)[0] != 0 and "bad arguments" in _last_error(lib)
    assert _call(lib, dense=[b"a", None, b"c"])[0] != 0 and "dense text 1" in _last_error(lib)
    assert _call(lib, dense_lens=[1, -1, 1])[0] != 0 and "dense text 1" in _last_error(lib)
    assert _call(lib, sparse_lens=[1, 1, -2])[0] != 0 and "sparse text 2" in _last_error(lib)
