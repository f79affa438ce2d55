"""CPU tier of the family every-row tests (encoder_family_rows_case.py), on oracle output alone: the route helpers restate
csrc/encoder.hip, span_batch holds what it promises, the oracles' new keywords change no bit, and — the point — every
mistake of the catalogue, planted in the oracle, moves an exposed row of every sequence longer than 16 tokens by more
than twice the f16 bar, while f16 operands alone stay inside half of it. The figures this file prints are the ones
recorded in profiles/encoder_family_rows_checks.md."""
import numpy as np
import pytest

import qwen2_oracle as qo
import t5_oracle as t5
from encoder_family_rows_case import (FAMILIES, MISTAKES, SPAN_LENS, WIDTHS, family_route_edges, model, movement, skinny_route,
                                      span_batch, token_index, token_spans)
from encoder_rows_case import FIXED_EDGES, mid_threshold, route_edges
from rope_oracle import f16_operand
from test_encoder_gpu import TOL

CASES = [(f, H) for f in FAMILIES for H in WIDTHS] + [("qwen2", 896)]


# ---- routes ----------------------------------------------------------------------------------------------------------------
def _mid_usable(M, N, n_cu):
    """mid_usable of csrc/encoder.hip for the shapes of these tests (K % 32 == 0, N % 8 == 0), n_cu as
    launch_gemm_f16x3 rounds it."""
    return M > 256 and 4 * (-(-M // 256)) * (-(-N // 256)) <= n_cu // 8 * 8


def _skinny_routed(M, N, K):
    """skinny_routed of csrc/encoder.hip, written out a second time."""
    sk_waves = 8 if K % 256 == 0 else 4 if K % 128 == 0 else 0
    sk_steps = K // (32 * sk_waves) if sk_waves else 0
    one_launch = sk_steps > 0 and (sk_steps % 6 == 0 or sk_steps % 4 == 0 or sk_steps % 3 == 0) and N % 16 == 0
    slice_ = next((c for c in (192, 256, 128, 64, 32) if K % c == 0), 0)
    return M <= 256 and (one_launch or (slice_ > 0 and N % 64 == 0))


@pytest.mark.parametrize("n_cu", [256, 304, 64, 60])
@pytest.mark.parametrize("family,H", CASES)
def test_family_route_edges_straddle_the_mid_kernel_limit_on_any_device(family, H, n_cu):
    m = model(family, H)
    assert m.Ns == ((H, 3 * H, 4 * H) if family != "t5" else (H, 3 * H, 2 * H))
    edges = family_route_edges(m.Ns, n_cu)
    assert edges == sorted(set(edges)) and set(FIXED_EDGES) <= set(edges)
    assert edges == route_edges(H, m.N1, n_cu)  # (the generalisation agrees with the helper it generalises)
    for N in m.Ns:
        thr = mid_threshold(N, n_cu)
        if thr == 0:
            assert not any(_mid_usable(M, N, n_cu) for M in (257, 512, 513, 4096))
            continue
        assert thr % 256 == 0 and thr in edges and thr + 1 in edges
        assert not _mid_usable(thr + 1, N, n_cu)
        assert _mid_usable(thr, N, n_cu) if thr > 256 else thr == 256
    for e in edges:  # nothing but the fixed edges and the thresholds
        assert e in FIXED_EDGES or any(e - d == mid_threshold(N, n_cu) for N in m.Ns for d in (0, 1))


def test_the_ladder_at_256_compute_units():
    """DESIGN.md section 4, 'Every-row tests of the other families': the last M on the mid kernel per N."""
    assert [mid_threshold(N, 256) for N in (384, 1152, 1536)] == [8192, 3072, 2560]      # H = 384, gated
    assert [mid_threshold(N, 256) for N in (768, 2304, 3072)] == [5376, 1792, 1280]      # H = 768, gated
    assert [mid_threshold(N, 256) for N in (896, 2688, 3584)] == [4096, 1280, 1024]      # Qwen2 at 896
    assert mid_threshold(768, 256) == 5376 and mid_threshold(1536, 256) == 2560          # T5: I = 2H
    assert max(family_route_edges((384, 1152, 1536), 256)) == 8193


@pytest.mark.parametrize("M", [1, 16, 17, 64, 65, 255, 256, 257])
def test_skinny_routes_of_the_widths(M):
    """Which skinny kernel the rotary / gate epilogues run in, per K, while M <= 256: one launch at K = 384 (4 waves x 3
    steps), 768 (8 x 3), 1024 (8 x 4) and 1536 (8 x 6); the two-launch split-K route at K = 896 (4 waves x 7 steps) and
    K = 1792 (8 x 7), where 7 steps admit no unroll of 6, 4 or 3 — both of Qwen2-896's products."""
    inside = M <= 256
    for K, N in ((384, 1152), (384, 1536), (768, 2304), (768, 3072), (1024, 3072), (1536, 768), (768, 384)):
        assert skinny_route(M, N, K) == ("one" if inside else None), (K, N)
        assert _skinny_routed(M, N, K) == inside
    for K, N in ((896, 2688), (896, 3584), (1792, 896)):
        assert skinny_route(M, N, K) == ("split" if inside else None), (K, N)
        assert _skinny_routed(M, N, K) == inside
    for K, N in ((384, 1152), (896, 2688), (1792, 896), (800, 64), (896, 2690)):
        assert (skinny_route(M, N, K) is not None) == _skinny_routed(M, N, K)


# ---- the builder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 16, 17, 64, 255, 256, 257, 487, 488, 974, 1025, 2561, 8193])
def test_span_batch_returns_exactly_what_was_asked(T):
    seqs, which = span_batch(T)
    assert sum(len(s) for s in seqs) == T and len(seqs) == len(which)
    assert all(1 <= len(s) <= max(SPAN_LENS) and 0 <= int(s.min()) and int(s.max()) < 64 for s in seqs)
    first = {}
    for s, j in zip(seqs, which.tolist()):
        assert np.array_equal(first.setdefault(j, s), s)                     # equal index, equal tokens
        assert j == 11 or len(s) == SPAN_LENS[j % len(SPAN_LENS)]
    assert len({s.tobytes() for s in first.values()}) == len(first)          # distinct index, distinct tokens
    ids, off, span_off, span_tok = token_spans(seqs)
    assert len(ids) == T == span_off[-1] == len(span_tok) and np.array_equal(off, span_off)
    inside = np.concatenate([np.arange(len(s)) for s in seqs])
    assert np.array_equal(span_tok[:, 0], inside) and np.array_equal(span_tok[:, 1], inside + 1)  # every token, once
    distinct, row = token_index(seqs, which)
    flat = np.concatenate(distinct)
    assert len(row) == T and np.array_equal(flat[row], ids)
    assert len(np.unique(row)) == len(flat)                                  # every token of every distinct sequence
    if T >= 2 * 487:  # two cycles: every one of the 11 repeats, at another offset inside a 128-row panel
        starts = off[:-1]
        for j in range(11):
            assert len({int(o) % 128 for o in starts[which == j]}) >= 2, j


# ---- the oracles' new keywords ---------------------------------------------------------------------------------------------
def test_the_new_keywords_change_no_bit():
    """hooks=None / operand=None are the oracles as they were: test_*_cpu.py pin every one of them to its library's
    goldens at 1e-9 with those defaults. Here: an empty hooks dict is the default too, and T5's operand= with the
    identity is bit-identical to none."""
    seq = span_batch(300)[0][2]
    for family in FAMILIES:
        m = model(family, 384)
        assert np.array_equal(m.hidden(seq), m.hidden(seq, hooks={})), family
    m = model("t5", 384)
    assert np.array_equal(m.hidden(seq), t5.encode_one(m.w, m.shape, seq, operand=lambda a: a))
    assert np.array_equal(m.hidden(seq), t5.encode_one(m.w, m.shape, seq))  # (and f64_weights changes none)


# ---- the catalogue ---------------------------------------------------------------------------------------------------------
def _long_sequences():
    seqs, which = span_batch(487)
    return [s for s in seqs if len(s) > 16]


@pytest.mark.parametrize("family,H", CASES)
def test_every_mistake_moves_a_row_and_f16_operands_do_not(family, H):
    """Per family and width, on the sequences of span_batch longer than 16 tokens: (2) the oracle with f16 operands stays
    within TOL['f16'][1] / 2 of the f64 rows, on every row; (1) every mistake of the catalogue that applies moves at least
    one row of every such sequence by more than 2 TOL['f16'][1]. Nothing is exempt: a mistake that cannot be seen fails
    here."""
    m = model(family, H)
    bar = TOL["f16"][1]
    seqs = _long_sequences()
    assert sorted(len(s) for s in seqs) == [17, 17, 63, 63, 64, 64, 65, 129]
    noise = [movement(m.hidden(s, operand=f16_operand), m.states(s)) for s in seqs]
    worst_cos, worst_abs = max(c.max() for c, _ in noise), max(a.max() for _, a in noise)
    print(f"{m.name}: f16 operands, worst |1-cos| = {worst_cos:.3e}, worst abs = {worst_abs:.3e} (half the bar: {bar / 2:.1e})")
    assert worst_abs < bar / 2 and worst_cos < TOL["f16"][0] / 2
    applied, unseen = 0, []
    for name, (applies, what) in MISTAKES.items():
        if not applies(m):
            continue
        applied += 1
        best = [movement(m.hidden(s, **what(m)), m.states(s))[1].max() for s in seqs]  # per sequence: its most moved row
        print(f"{m.name}: {name}: the most moved row of a sequence moves by {min(best):.3e} .. {max(best):.3e}")
        if not min(best) > 2 * bar:
            unseen.append((name, min(best)))
    assert not unseen, unseen
    expected = {"nomic-silu": 11, "nomic-gelu": 11, "alibi": 7, "modernbert": 13, "t5": 6, "qwen2": 14}
    assert applied == expected[family]


def test_rotation_mistakes_leave_the_causal_first_row_alone():
    """Qwen2's row 0 sees only itself at position 0: no rotation mistake can move it, exactly — which is why one-token
    sequences say nothing about a rotation."""
    m = model("qwen2", 384)
    seq = _long_sequences()[0]
    for name, (applies, what) in MISTAKES.items():
        if name.startswith("rotation") and applies(m):
            assert np.array_equal(m.hidden(seq, **what(m))[0], m.states(seq)[0]), name
    assert qo.encode_one(m.w64, m.shape, seq[:1]).shape == (1, 384)
