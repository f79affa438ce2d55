"""The planted shadow-bound cases (tests/shadow_bounds.py), proven on the CPU from the f64 model and the oracle alone:
the model's constants are the sources', its bound is sound on random data and almost unused there, and every case of
the GPU matrix (test_shadow_bounds_gpu.py) (1) realises the stated fraction of its bound, (2) keeps the oracle's top k
among the candidates of the documented bound, (3) stays under the candidate cap that keeps the GPU tests away from the
overflow fallbacks, and (4) loses a planted winner under every mistake of the catalogue it claims.
Each case prints one `SHADOW|` line (profiles/shadow_bounds_checks.md is made from them)."""
import json
import os

import numpy as np
import pytest

import search_layouts as sl
import shadow_bounds as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voitta_rag_amd", "csrc")


def _log(**kw):
    print("SHADOW| " + json.dumps(kw))


def test_model_constants_are_the_sources():
    text = {}
    for name, line in sb.SOURCE_LINES:
        if name not in text:
            with open(os.path.join(CSRC, name)) as f:
                text[name] = f.read()
        assert line in text[name], (name, line)
    assert sb.CENTRE_MIN_ROWS == 1024 and sb.CAND_CAP_BATCHED < sl.kBatchCand and sb.CAND_CAP_SINGLE < sl.kMaxCandTiles


@pytest.mark.parametrize("form,dim,centred,batched", [("int8", 128, False, False), ("int8", 128, True, False),
                                                      ("int8", 384, True, True), ("f16", 96, False, False),
                                                      ("f16", 256, False, False)])
def test_the_documented_bound_is_sound_and_random_data_leaves_it_unused(form, dim, centred, batched):
    """|f - A| <= E for every row in f64, and over random queries near stored rows the largest |f - A| / E stays below
    a half: what the planted cases are for."""
    rng = np.random.default_rng(dim)
    xh = sb.prep(sb.background(4224, dim, 7).astype(np.float32))
    sh = sb.Shadow(form, xh, xh.mean(0) + 0.05 * sb.unit(rng.standard_normal(dim)) if centred else None)
    worst = 0.0
    for _ in range(8):
        qh = sb.prep(sb.unit(xh[rng.integers(4224)] + 0.5 * sb.unit(rng.standard_normal(dim))).astype(np.float32))[0]
        b = sb.bounds(sh, qh, batched)
        worst = max(worst, float(np.max(np.abs(sh.exact(qh) - b.A) / b.E)))
    assert worst < 0.5, worst
    _log(check="random-data", form=form, dim=dim, centred=centred, batched=batched, largest_realised=round(worst, 3))


def test_degenerate_rows_in_the_model():
    x = sb.background(8, 64, 1).astype(np.float32)
    x[1] = 0.0
    x[2] *= 1e-4
    x[3, 5] = np.inf
    x[4, 6] = np.nan
    sh = sb.Shadow("int8", sb.prep(x))
    assert sh.s[1] == 0 and sh.err[1] == pytest.approx(1e-12) and sh.s[2] < 1e-6 and np.isinf(sh.err[[3, 4]]).all()
    assert sb.centre_after(sb.prep(np.repeat(x, 256, 0)), [2048])[0] is None  # a non-finite column sum: no centre
    b = sb.bounds(sh, sb.prep(x[:1])[0])
    assert set(sb.candidates(b, 1)) == {0, 3, 4}  # rows without a finite bound are always candidates
    assert set(sb.candidates(b, 1, np.array([1, 1, 1, 0, 0, 1, 1, 1], bool))) == {0}


def test_centre_follows_the_doubling_rule():
    xh = sb.prep(sb.background(5000, 16, 3).astype(np.float32))
    c = sb.centre_after(xh, [700, 300, 24, 1000, 24, 2000])
    assert c[0] is None and c[1] is None and np.allclose(c[2], xh[:1024].mean(0)) and c[3] is c[2]
    assert np.allclose(c[4], xh[:2048].mean(0)) and c[5] is c[4]
    assert all(v is None for v in sb.centre_after(xh, [4096, 4096], centring=False))


def test_edge_rows_are_where_they_say():
    rows = sb.edge_rows(sb.N_TAIL15)
    slot, visit = sl.row_slots(sb.N_TAIL15)
    assert [rows[f"pos{p}"] % 16 for p in range(16)] == list(range(16)) and len({rows[f"pos{p}"] // 16 for p in range(16)}) == 1
    assert rows["tail_last_row"] == sb.N_TAIL15 - 1 and rows["tail_first_row"] % 16 == 0 and sb.N_TAIL15 - rows["tail_first_row"] == 15
    assert slot[rows["block_first_tile"]] % sl.kScanWaves == 0 and slot[rows["block_last_tile"]] % sl.kScanWaves == sl.kScanWaves - 1
    assert slot[rows["block_first_tile"]] // sl.kScanWaves == slot[rows["block_last_tile"]] // sl.kScanWaves
    assert "grid_stride_tile" not in rows  # 265 tiles on 34 blocks: no wave walks twice
    big = sb.edge_rows(sl.N_GRID_STRIDE)
    assert sl.row_slots(sl.N_GRID_STRIDE)[1][big["grid_stride_tile"]] >= sl.kTileRows
    for name, row in sb.BATCH_W_ROWS.items():
        assert (row % 256 < 128) == (name == "first_slab") or name == "partial_tile"
    assert sb.N_BATCH % 16 == 1 and sb.BATCH_W_ROWS["partial_tile"] == sb.N_BATCH - 1


def _check(name, kw, centring):
    case = sb.plant(centring, **kw)
    frac, cand, missed = sb.check_case(case, centring)
    rows, _ = case.oracle_topk()
    floor, cap = sb.realised_floor(case), sb.CAND_CAP_BATCHED if case.batched else sb.CAND_CAP_SINGLE
    _log(case=name, centring=centring, realised=round(frac, 3), floor=floor, candidates=int(cand.shape[0]), k=case.k)
    assert np.isin(case.winners, rows).all(), (name, "a planted winner is not in the oracle's top k")
    assert frac >= floor, (name, frac)                      # (1)
    assert np.isin(rows, cand).all(), name                   # (2)
    assert cand.shape[0] <= cap, (name, cand.shape[0])       # (3)
    assert missed == [], (name, missed)                      # (4)
    return case


INT8 = sb.single_cases("int8") + sb.batched_cases()
F16 = sb.single_cases("f16")


@pytest.mark.parametrize("centring", [True, False], ids=["centred", "uncentred"])
@pytest.mark.parametrize("name,kw", INT8, ids=[c[0] for c in INT8])
def test_int8_case(name, kw, centring):
    _check(name, kw, centring)


@pytest.mark.parametrize("name,kw", F16, ids=[c[0] for c in F16])
def test_f16_case(name, kw):
    """The f16 form reaches 0.8 of E at D = 96 only (starved winner 0.809). Reached elsewhere: D = 96 inflated 0.752,
    D = 256 0.750 / 0.711, D = 288 0.731 / 0.714 (starved / inflated): c_fixed = D 5e-7 is a quarter of the largest
    possible E there and no input realises it. Each is held to the reached figure minus 0.05 (sb.REALISED_FLOOR_F16)."""
    case = _check(name, kw, True)
    sub = np.abs(sb.prep(case.x[case.planted])) < 2.0 ** -14
    assert (sub & (sb.prep(case.x[case.planted]) != 0)).sum(1).min() >= 4  # components below the f16 normal range


def test_matrix_covers_the_stated_shapes():
    names = [c[0] for c in INT8 + F16]
    assert len(set(names)) == len(names)
    for dim in sb.INT8_DIMS:
        assert {f"int8-d{dim}-starved-n{sb.N_TAIL15}-k{k}" for k in sb.STARVED_K} <= set(names)
    assert {f"int8-d128-starved-k10-pos{p}" for p in range(16)} <= set(names)
    assert {f"f16-d96-starved-k10-pos{p}" for p in range(16)} <= set(names)
    assert "int8-d128-starved-k10-grid_stride_tile" in names and "int8-d128-starved-k10-tail_one_row" in names
    assert sb.N_TAIL15 % 16 == 15 and sb.N_TAIL1 % 16 == 1 and [d // 64 for d in sb.INT8_DIMS] == [2, 6, 7]
    assert [d // 32 for d in sb.F16_DIMS[1:]] == [8, 9] and sb.F16_DIMS[0] % 64 != 0
    # k = 64 cannot be planted under the cap: W and 64 decoys are 65 candidates
    assert max(sb.STARVED_K) + 1 == sb.CAND_CAP_SINGLE and 2 * max(sb.INFLATED_K) == sb.CAND_CAP_SINGLE


@pytest.mark.parametrize("stage", ["before", "after"])
@pytest.mark.parametrize("dim", [128, 384])
def test_drifted_centre_case(dim, stage):
    """W lives in the part appended after the first centring; asked before the doubling its bytes are those of the old
    centre, asked after it those of the new one. Pairing them with the err_r of the other centre, or leaving the clamp
    out where the residual exceeds the row's own largest component, drops W."""
    case = sb.plant_drifted_centre(dim, 10, stage=stage)
    mistakes, sh = sb.stale_centre_mistakes(case)
    b = sb.bounds(sh, case.qh)
    cand = sb.candidates(b, case.k)
    rows, _ = case.oracle_topk()
    frac = case.realised(sh, b)
    _log(case=f"drift-d{dim}-{stage}", realised=round(frac, 3), candidates=int(cand.shape[0]), centre_norm=round(sh.cn, 3))
    assert rows[0] == case.winners[0] and frac >= sb.REALISED_MIN and np.isin(rows, cand).all() and cand.shape[0] <= sb.CAND_CAP_SINGLE
    w = case.winners[0]
    assert np.abs(sh.r[w]).max() > np.abs(sh.xh[w]).max()  # the residual exceeds the row's own maximum
    assert set(mistakes) == ({"err_of_current_centre_bytes_of_old"} if stage == "before" else
                             {"err_of_old_centre_bytes_of_current", "clamp_missing"})
    for name, (shadow, kwargs) in mistakes.items():
        assert sb.detects(case, shadow, kwargs), (dim, stage, name)
    assert set(sb.CENTRE_MISTAKES) == {"err_of_current_centre_bytes_of_old", "err_of_old_centre_bytes_of_current", "clamp_missing"}


def test_mistakes_not_covered_are_named_in_the_design_document():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    for name in sb.NOT_COVERED:
        assert name in design, name
    # which cases happen to see them (recorded, never claimed)
    seen = {name: 0 for name in sb.NOT_COVERED}
    picks = [c for c in INT8 if c[0].endswith(("-k1", "-k10", "-k63", "-k32", "first_slab", "inflated"))]
    for _, kw in picks:
        case = sb.plant(True, **kw)
        sh = case.shadow(True)
        for name, f in sb.NOT_COVERED.items():
            seen[name] += sb.detects(case, sh, f(sh))
    _log(check="not-covered", cases=len(picks), seen=seen)
    assert all(v < len(picks) for v in seen.values())  # none of them is seen by every case: nothing to claim
