"""The two-stage dense searches on rows that use the whole error bound (tests/shadow_bounds.py): a starved winner whose
shadow underestimates it by most of E, an inflated threshold whose impostors are overestimated by most of E, at every
in-tile position, tile and block edge, on the int8 scan (prefilter_scan8_kernel), the f16 scan (prefilter_scan_kernel)
and the batched search (batch.hip), and after every step that rebuilds or moves the derived data.
Every assertion is "rows and f32 score bits equal oracle.core's on the final corpus"; beside it each test checks on
Engine.stats() that the path under test answered (two_stage / batched rose), that no overflow fallback did, and that
the candidates stay within what the f64 model allows with E doubled, plus k: a bound that is sound but vacuous fails
there. The CPU model proves what each case is for (test_shadow_bounds_cpu.py); it is never the expected answer.
Each case prints one `SHADOW|` line (profiles/shadow_bounds_checks.md is made from them)."""
import json
import os

import numpy as np
import pytest

import search_layouts as sl
import shadow_bounds as sb
from oracle import core as ocore

pytestmark = pytest.mark.gpu


def _engine(dim, **kw):
    from voitta_rag_amd import Engine

    return Engine(dim, **kw)


def _log(**kw):
    print("SHADOW| " + json.dumps(kw))


def _want(x, q, k, live=None):
    sc = sl.reference_scores(x, q)[0]
    return ocore.topk(sc, k, None if live is None else np.asarray(live, np.uint8))


def _cap(sh, q, k, live=None, batched=False):
    """candidates of the documented bound with E doubled, plus k: the most the engine may re-score"""
    b = sb.bounds(sh, sb.prep(q)[0], batched)
    return int(sb.candidates(b, k, live, batched, widen=2.0).shape[0]) + k


def _ask(e, x, q, k, sh, live=None, tag=None):
    """one single-query search against the oracle on the corpus x (live: rows not deleted) -> last_candidates"""
    before = e.stats()
    rows, scores = e.search_dense(np.asarray(q, np.float32).reshape(1, -1), k)[0]
    after = e.stats()
    wr, ws = _want(x, q, k, live)
    assert np.array_equal(rows, wr), (tag, rows, wr)
    assert np.array_equal(scores.view(np.uint32), ws.view(np.uint32)), tag
    assert after["two_stage"] - before["two_stage"] == 1 and after["fallback"] == before["fallback"], (tag, before, after)
    cap = _cap(sh, q, k, live)
    assert 0 <= after["last_candidates"] <= cap, (tag, after["last_candidates"], cap)
    return after["last_candidates"], cap


def _centring(monkeypatch, centring):
    if centring:
        monkeypatch.delenv("VR_PREFILTER_CENTRE", raising=False)
    else:
        monkeypatch.setenv("VR_PREFILTER_CENTRE", "0")


def _single(name, kw, centring):
    case = sb.plant(centring, **kw)
    sh = case.shadow(centring)
    e = _engine(case.x.shape[1])
    assert e.upsert(case.x) == 0
    got, cap = _ask(e, case.x, case.q, case.k, sh, tag=name)
    assert np.isin(case.winners, _want(case.x, case.q, case.k)[0]).all(), name
    _log(case=name, centring=centring, k=case.k, last_candidates=got, model_cap=cap)
    e.close()


INT8 = sb.single_cases("int8")
F16 = sb.single_cases("f16")
BATCHED = sb.batched_cases()


@pytest.mark.parametrize("centring", [True, False], ids=["centred", "uncentred"])
@pytest.mark.parametrize("name,kw", INT8, ids=[c[0] for c in INT8])
def test_int8_single_query(gpu, name, kw, centring, monkeypatch):
    """prefilter_scan8_kernel: kb8n = 2, 6, 7; the planted row at all 16 in-tile positions, in the partial last tile,
    in the first and last tile of a scan block and in a tile only the grid-stride walk reaches; k = 1, 10, 63 (32)."""
    _centring(monkeypatch, centring)
    _single(name, kw, centring)


@pytest.mark.parametrize("name,kw", F16, ids=[c[0] for c in F16])
def test_f16_single_query(gpu, name, kw, monkeypatch):
    """prefilter_scan_kernel: dim 96 has no other form; 256 and 288 with VR_PREFILTER=f16 (set before the engine exists)"""
    if kw["dim"] % 64 == 0:
        monkeypatch.setenv("VR_PREFILTER", "f16")
    _single(name, kw, True)


# ---- the batched search -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nq", [17, 129])
@pytest.mark.parametrize("name,kw", BATCHED, ids=[c[0] for c in BATCHED])
def test_batched(gpu, name, kw, nq):
    """batch_scan_kernel / batch_pairs_kernel: the planted query at columns 0, 15, 16 and nq - 1 of a batch of Gaussian
    riders, W in the first and the last 128-row slab of a 256-row block and in the last partial tile; once more through
    search_dense_multi with W passing only the filter class of its own query (bit planes, the revisit's plane test);
    the planted query asked alone returns the same bits."""
    from voitta_rag_amd import SearchFilter

    case = sb.plant(True, **kw)
    n, dim = case.x.shape
    k = case.k
    sh = case.shadow(True)
    riders = sl.gaussian(nq, dim, 900 + nq)
    sc_riders = sl.reference_scores(case.x, riders)
    b_riders = [sb.bounds(sh, sb.prep(riders[i])[0], True) for i in range(nq)]
    b_planted = sb.bounds(sh, case.qh, True)

    def cap(b, live=None):
        return int(sb.candidates(b, k, live, True, widen=2.0).shape[0]) + k

    caps = np.array([cap(b) for b in b_riders])
    cap_planted = cap(b_planted)
    rng = np.random.default_rng(nq)
    folder = np.zeros(n, np.int32)
    folder[rng.choice(n, n // 20, replace=False)] = 9
    special = np.concatenate([case.planted, case.winners])
    folder[special] = 7
    e = _engine(dim)
    e.upsert(case.x, folder_ids=folder)
    want_planted = _want(case.x, case.q, k)
    assert np.isin(case.winners, want_planted[0]).all()
    log = {}
    for col in (0, 15, 16, nq - 1):
        q = riders.copy()
        q[col] = case.q
        before = e.stats()
        got = e.search_dense(q, k)
        after = e.stats()
        for i in range(nq):
            wr, ws = want_planted if i == col else ocore.topk(sc_riders[i], k)
            assert np.array_equal(got[i][0], wr), (name, nq, col, i)
            assert np.array_equal(got[i][1].view(np.uint32), ws.view(np.uint32)), (name, nq, col, i)
        assert after["batched"] - before["batched"] == nq and after["batch_fallback"] == before["batch_fallback"], (name, col)
        assert after["two_stage"] == before["two_stage"] and after["fallback"] == before["fallback"], (name, col)
        total, allowed = after["batch_candidates"] - before["batch_candidates"], int(caps.sum() - caps[col] + cap_planted)
        assert total <= allowed, (name, nq, col, total, allowed)
        log[col] = total
        alone = e.search_dense(q[col:col + 1], k)[0]
        assert np.array_equal(alone[0], got[col][0]) and np.array_equal(alone[1].view(np.uint32), got[col][1].view(np.uint32))
    # a filter per query: the planted rows pass only in the class of the planted query
    col = 16
    q = riders.copy()
    q[col] = case.q
    own, others = SearchFilter(exclude_folders=[9]), SearchFilter(exclude_folders=[7])
    masks = {True: folder != 9, False: folder != 7}
    before = e.stats()
    got = e.search_dense_multi(q, k, [own if i == col else others for i in range(nq)])
    after = e.stats()
    sc_planted = sl.reference_scores(case.x, case.q)[0]
    for i in range(nq):
        wr, ws = ocore.topk(sc_planted if i == col else sc_riders[i], k, masks[i == col].astype(np.uint8))
        assert np.array_equal(got[i][0], wr), (name, nq, "multi", i)
        assert np.array_equal(got[i][1].view(np.uint32), ws.view(np.uint32)), (name, nq, "multi", i)
    assert np.isin(case.winners, got[col][0]).all() and not np.isin(special, np.concatenate([got[i][0] for i in range(nq) if i != col])).any()
    assert after["batched"] - before["batched"] == nq and after["batch_fallback"] == before["batch_fallback"], (name, "multi")
    allowed = sum(cap(b_planted if i == col else b_riders[i], masks[i == col]) for i in range(nq))
    total = after["batch_candidates"] - before["batch_candidates"]
    _log(case=name, nq=nq, k=k, batch_candidates_by_column=log, model_cap=int(caps.sum() - caps[0] + cap_planted),
         multi_candidates=total, multi_cap=allowed)
    assert total <= allowed, (name, "multi", total, allowed)
    e.close()


# ---- derived data after every step that rebuilds or moves it -----------------------------------------------------------------

@pytest.mark.parametrize("centring", [True, False], ids=["centred", "uncentred"])
def test_planted_question_after_every_rebuild(gpu, centring, monkeypatch, tmp_path):
    """One engine, one search lane, the starved winner asked after: the first upsert; an upsert that grows the capacity
    (no re-centring: the collection has not doubled); delete_rows of the best decoy (the tombstone must show); compact()
    (rows renumbered, the shadow rebuilt around the survivors' mean); save and load into a fresh engine (shadow rebuilt);
    one more upsert there. Uncentred, W uses most of its bound at every step; centred, up to the compaction (afterwards
    the centre has moved and W is an ordinary spiky row: the fraction is recorded)."""
    _centring(monkeypatch, centring)
    dim, k, n0 = 128, 10, sb.N_TAIL15
    case = sb.plant(centring, kind="starved", form="int8", n=n0, dim=dim, k=k, w_row=sb.W_MID)
    extra = sb.background(700, dim, 77).astype(np.float32)
    more = sb.background(100, dim, 78).astype(np.float32)
    x_all = np.concatenate([case.x, extra])
    xh_all = sb.prep(x_all)
    w = int(case.winners[0])
    steps = []

    def ask(e, x, shadow, live, step, at=w):
        got, cap = _ask(e, x, case.q, k, shadow, live, tag=step)
        b = sb.bounds(shadow, case.qh)
        frac = float((shadow.exact(case.qh)[at] - b.A[at]) / b.E[at])
        steps.append(dict(step=step, last_candidates=got, model_cap=cap, realised=round(frac, 3)))
        return frac

    e = _engine(dim, initial_rows=n0)
    e.upsert(case.x)
    c0 = sb.centre_after(xh_all, [n0, 700], centring)
    assert (c0[0] is None) == (not centring) and c0[1] is c0[0]
    assert ask(e, case.x, sb.Shadow("int8", xh_all[:n0], c0[0]), None, "first upsert") >= sb.REALISED_MIN
    e.upsert(extra)
    sh1 = sb.Shadow("int8", xh_all, c0[1])
    assert ask(e, x_all, sh1, None, "upsert that grows capacity") >= sb.REALISED_MIN
    live_all = np.ones(x_all.shape[0], bool)
    live_all[case.decoys[0]] = False
    e.delete_rows(case.decoys[:1])
    assert ask(e, x_all, sh1, live_all, "delete_rows of a decoy") >= sb.REALISED_MIN
    assert case.decoys[0] in _want(x_all, case.q, k)[0] and case.decoys[0] not in _want(x_all, case.q, k, live_all)[0]
    remap = e.compact()
    assert remap[case.decoys[0]] == -1 and (remap >= 0).sum() == live_all.sum()
    x_cur = x_all[live_all]
    sh2 = sb.Shadow("int8", sb.prep(x_cur), sb.rebuilt_centre(sb.prep(x_cur), centring))
    w_cur = int(remap[w])
    assert np.array_equal(x_cur[w_cur], x_all[w])
    frac = ask(e, x_cur, sh2, None, "compact", w_cur)
    assert frac >= sb.REALISED_MIN or centring
    path = os.path.join(str(tmp_path), "shadow.vrindex")
    e.save(path)
    e2 = _engine(dim)
    e2.load(path)
    ask(e2, x_cur, sh2, None, "save and load", w_cur)
    e2.upsert(more)
    x_fin = np.concatenate([x_cur, more])
    sh3 = sb.Shadow("int8", sb.prep(x_fin), sh2.centre)
    ask(e2, x_fin, sh3, None, "upsert after load", w_cur)
    ask(e, x_cur, sh2, None, "the first engine again", w_cur)
    _log(case="lifecycle", centring=centring, steps=steps)
    e.close()
    e2.close()


@pytest.mark.parametrize("centring", [True, False], ids=["centred", "uncentred"])
@pytest.mark.parametrize("stage", ["before", "after"])
@pytest.mark.parametrize("dim", [128, 384])
def test_drifted_centre(gpu, dim, stage, centring, monkeypatch):
    """2,112 rows around a common direction, 2,111 Gaussian rows appended against the first part's centre, two more that
    cross the doubling: the question is asked before and after the re-centring. The case of stage "before" uses its
    bound under the old centre, the one of stage "after" under the new one (uncentred: exactness only)."""
    _centring(monkeypatch, centring)
    case = sb.plant_drifted_centre(dim, 10, stage=stage, centring=centring)
    x = case.all_rows
    xh = sb.prep(x)
    centres = sb.centre_after(xh, case.upserts, centring)
    e = _engine(dim)
    at, log = 0, []
    for i, m in enumerate(case.upserts):
        e.upsert(x[at:at + m])
        at += m
        if at < sl.PREFILTER_MIN_ROWS:
            continue
        sh = sb.Shadow("int8", xh[:at], centres[i])
        got, cap = _ask(e, x[:at], case.q, case.k, sh, tag=(dim, stage, at))
        b = sb.bounds(sh, case.qh)
        w = case.winners[0]
        frac = float((sh.exact(case.qh)[w] - b.A[w]) / b.E[w])
        if at == case.asked and centring:
            assert frac >= sb.REALISED_MIN, (dim, stage, frac)
        log.append(dict(rows=at, last_candidates=got, model_cap=cap, realised=round(frac, 3)))
    assert len(log) == 2
    _log(case=f"drift-d{dim}-{stage}", centring=centring, asks=log)
    e.close()


def test_degenerate_bystanders(gpu):
    """A zero row, a row of norm 1e-4 (the keep rule stores it unnormalised: a tiny scale), a row holding inf and one
    holding NaN, the last two deleted before any search. They enter the column sums, so the engine has no centre (the
    case is planted for none); the planted question comes out exact from the two-stage path, again after a further
    upsert. No rank of a non-finite row is asserted."""
    dim, k = 128, 10
    case = sb.plant(False, kind="starved", form="int8", n=sb.N_TAIL15, dim=dim, k=k, w_row=sb.W_MID)
    x = case.x.copy()
    zero, tiny, inf, nan = 300, 301, 1100, 3001
    assert not np.isin([zero, tiny, inf, nan], np.concatenate([case.decoys, case.winners])).any()
    x[zero] = 0.0
    x[tiny] *= 1.0e-4
    x[inf, 3] = np.inf
    x[nan, 5] = np.nan
    xh = sb.prep(x)
    assert sb.rebuilt_centre(xh) is None and np.array_equal(xh[tiny].astype(np.float32), x[tiny])
    live = np.ones(x.shape[0], bool)
    live[[inf, nan]] = False
    e = _engine(dim)
    e.upsert(x)
    e.delete_rows([inf, nan])
    sh = sb.Shadow("int8", xh, None)
    assert np.isinf(sh.err[[inf, nan]]).all() and sh.s[zero] == 0 and 0 < sh.s[tiny] < 1e-6
    got, cap = _ask(e, x, case.q, k, sh, live, tag="degenerate")
    more = sb.background(64, dim, 5).astype(np.float32)
    e.upsert(more)
    x2 = np.concatenate([x, more])
    live2 = np.concatenate([live, np.ones(64, bool)])
    got2, cap2 = _ask(e, x2, case.q, k, sb.Shadow("int8", sb.prep(x2), None), live2, tag="degenerate + upsert")
    _log(case="degenerate", last_candidates=[got, got2], model_cap=[cap, cap2])
    e.close()
