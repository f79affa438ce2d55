"""No-GPU checks of the filtered batches (vr_search_dense_multi / vr_search_hybrid_batch_multi): the library exports
both, the ctypes table declares them with the header's argument types, SearchFilter keys group equal filters, and
malformed input is rejected with a message before the engine is touched (a NULL engine: valid input reaches the
engine check, bad input never does)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vr_search_dense_multi", "vr_search_hybrid_batch_multi")


def test_library_exports_the_filtered_batches():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES


def _header_params(name):
    src = open(os.path.join(ROOT, "include", "voitta_engine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
    assert m, name
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def _ctype_of(param):
    from voitta_rag_amd import _lib

    t = param.rsplit(" ", 1)[0].replace("const ", "").strip()
    ptr = param.count("*")
    t = t.replace("*", "").strip()
    base = {"int32_t": C.c_int32, "int64_t": C.c_int64, "int": C.c_int, "float": C.c_float, "double": C.c_double,
           "vr_filter": _lib.VrFilter}[t]
    return C.POINTER(base) if ptr else base


def test_ctypes_declarations_follow_the_header():
    from voitta_rag_amd import _lib

    for n in NAMES:
        params = _header_params(n)
        restype, argtypes = _lib.SIGNATURES[n]
        assert restype is C.c_int
        assert len(argtypes) == len(params), (n, params)
        for p, a in zip(params, argtypes):
            if p.startswith("vr_engine") or p.startswith("const float* q"):
                assert a is C.c_void_p, (n, p)  # (engine handle; queries may be a device pointer)
            else:
                assert a == _ctype_of(p), (n, p, a)


def test_filter_keys_group_equal_filters():
    from voitta_rag_amd import SearchFilter

    a = SearchFilter(include_folders=[3, 1, 1], exclude_folders=[7])
    b = SearchFilter(include_folders=[1, 3], exclude_folders=[7])
    assert a.key() == b.key() and hash(a.key()) == hash(b.key())
    assert SearchFilter().key() is None
    # the date field only matters with a date bound
    assert SearchFilter(date_field="created").key() is None
    assert SearchFilter(date_start=5, date_field="modified").key() == SearchFilter(date_start=5).key()
    different = [
        SearchFilter(include_folders=[1, 3]),
        SearchFilter(include_folders=[1]),
        SearchFilter(include_folders=[]),  # (an empty must-set passes nothing; no must-set passes everything)
        SearchFilter(folder_filter=1),
        SearchFilter(folder_filter=1, include_folders=[1]),
        SearchFilter(exclude_folders=[1]),
        SearchFilter(exclude_index_folders=[1]),
        SearchFilter(date_start=5),
        SearchFilter(date_end=5),
        SearchFilter(date_start=5, date_field="created"),
        SearchFilter(date_start=5, date_end=9),
    ]
    keys = [f.key() for f in different]
    assert len(set(keys)) == len(keys)


def _filters(n, **kw):
    from voitta_rag_amd import SearchFilter, _lib

    arr = (_lib.VrFilter * n)()
    keep = []
    for j in range(n):
        f, k = SearchFilter(exclude_folders=[j]).to_c()
        for name, v in kw.items():
            setattr(f, name, v)
        arr[j] = f
        keep.append(k)
    return arr, keep


def _last_error(lib):
    return lib.vr_last_error().decode()


def _dense_multi(lib, foq, n_filters=2, k=10, **kw):
    arr, keep = _filters(max(n_filters, 1), **kw)
    nq = len(foq)
    q = np.zeros((nq, 64), np.float32)
    rows = np.zeros((nq, k), np.int64)
    scores = np.zeros((nq, k), np.float32)
    counts = np.zeros(nq, np.int32)
    f = np.asarray(foq, np.int32)
    rc = lib.vr_search_dense_multi(None, C.c_void_p(q.ctypes.data), nq, 0, k, arr, n_filters,
                                   f.ctypes.data_as(C.POINTER(C.c_int32)), rows.ctypes.data_as(C.POINTER(C.c_int64)),
                                   scores.ctypes.data_as(C.POINTER(C.c_float)), counts.ctypes.data_as(C.POINTER(C.c_int32)))
    del keep
    return rc


def _hybrid_multi(lib, foq, limits, n_filters=2, out_stride=None, **kw):
    arr, keep = _filters(max(n_filters, 1), **kw)
    nq = len(foq)
    q = np.zeros((nq, 64), np.float32)
    lim = np.asarray(limits, np.int32)
    w = np.full(nq, 0.1, np.float64)
    stride = out_stride if out_stride is not None else max(1, int(lim.max()))
    rows = np.zeros((nq, max(stride, 1)), np.int64)
    scores = np.zeros((nq, max(stride, 1)), np.float64)
    fd = np.zeros((nq, max(stride, 1)), np.int32)
    counts = np.zeros(nq, np.int32)
    f = np.asarray(foq, np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    rc = lib.vr_search_hybrid_batch_multi(None, C.c_void_p(q.ctypes.data), nq, 0, None, None, None, p(lim, C.c_int32),
                                          p(w, C.c_double), 0, arr, n_filters, p(f, C.c_int32), stride, p(rows, C.c_int64),
                                          p(scores, C.c_double), p(fd, C.c_int32), p(counts, C.c_int32))
    del keep
    return rc


def test_valid_input_reaches_the_engine_check():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    assert _dense_multi(lib, [0, 1, -1]) != 0 and "null engine" in _last_error(lib)
    assert _hybrid_multi(lib, [0, 1, -1], [1, 21, 341]) != 0 and "null engine" in _last_error(lib)
    assert _hybrid_multi(lib, [-1, -1], [5, 5], n_filters=0) != 0 and "null engine" in _last_error(lib)


@pytest.mark.parametrize("foq", [[0, 2], [-2, 0], [0, 1 << 30]])
def test_filter_of_query_out_of_range(foq):
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    assert _dense_multi(lib, foq) != 0
    assert "filter_of_query" in _last_error(lib)
    assert _hybrid_multi(lib, foq, [10, 10]) != 0
    assert "filter_of_query" in _last_error(lib)


def test_malformed_filters_are_rejected():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    assert _dense_multi(lib, [0, 1], struct_size=8) != 0 and "size mismatch" in _last_error(lib)
    assert _hybrid_multi(lib, [0, 1], [10, 10], struct_size=1000) != 0 and "size mismatch" in _last_error(lib)
    assert _dense_multi(lib, [0, 1], n_must_folder_sets=3) != 0 and "must-sets" in _last_error(lib)
    assert _hybrid_multi(lib, [0, 1], [10, 10], n_must_folder_sets=-1) != 0 and "must-sets" in _last_error(lib)
    assert _dense_multi(lib, [0, 1], n_filters=-1) != 0 and "bad filters" in _last_error(lib)


@pytest.mark.parametrize("bad", [0, -3, 342, 1 << 20])
def test_limits_are_checked(bad):
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    assert _hybrid_multi(lib, [0, 1, -1], [10, bad, 10], out_stride=400) != 0
    assert "limits[1]" in _last_error(lib)


def test_out_stride_and_k_are_checked():
    from voitta_rag_amd import _lib

    lib = _lib.load_library()
    assert _hybrid_multi(lib, [0, 1], [10, 20], out_stride=19) != 0 and "out_stride" in _last_error(lib)
    assert _dense_multi(lib, [0, 1], k=0) != 0 and "k = 0" in _last_error(lib)
    assert _dense_multi(lib, [0, 1], k=1025) != 0 and "k = 1025" in _last_error(lib)
