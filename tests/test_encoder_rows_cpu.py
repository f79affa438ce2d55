"""CPU tier of the every-row encoder tests: the route-edge helper restates csrc/encoder.hip's thresholds correctly for
any CU count, the batch builders hold what they promise, and check_rows catches a single wrong row that the pooled
check of test_encoder_gpu lets through (shown on f64 oracle output alone, no GPU)."""
import numpy as np
import pytest

from encoder_rows_case import (FIXED_EDGES, RAGGED_LENS, check_rows, distinct_of, f64_weights, mid_threshold,
                               one_token_batch, ragged_batch, route_edges, three_token_batch)
from oracle import bert as obert


def test_route_edges_restate_the_table_for_256_compute_units():
    """DESIGN.md section 4, 'Every-row encoder tests': last M on the mid kernel for N = H, 3H, I."""
    table = {(384, 1536): (8192, 3072, 2560), (768, 3072): (5376, 1792, 1280), (1024, 4096): (4096, 1280, 1024)}
    for (H, I), thrs in table.items():
        edges = route_edges(H, I, 256)
        assert edges == sorted(set(edges))
        for e in FIXED_EDGES:
            assert e in edges
        for thr in thrs:
            assert thr in edges and thr + 1 in edges, (H, thr)
    e768 = route_edges(768, 3072, 256)
    for pair in ((1280, 1281), (1792, 1793), (5376, 5377)):
        assert pair[0] in e768 and pair[1] in e768


def _mid_usable(M, N, n_cu):
    """mid_usable of csrc/encoder.hip for the shapes of these tests (K % 32 == 0, N % 8 == 0), n_cu as
    launch_gemm_f16x3 rounds it."""
    return M > 256 and 4 * (-(-M // 256)) * (-(-N // 256)) <= n_cu // 8 * 8


@pytest.mark.parametrize("n_cu", [256, 304, 64, 60])
@pytest.mark.parametrize("H,I", [(384, 1536), (768, 3072), (1024, 4096)])
def test_route_edges_straddle_the_mid_kernel_limit_on_any_device(H, I, n_cu):
    edges = route_edges(H, I, n_cu)
    for N in (H, 3 * H, I):
        thr = mid_threshold(N, n_cu)
        if thr == 0:  # not even one 256-row tile per four CUs: no M takes the mid kernel, no edge to add
            assert not any(_mid_usable(M, N, n_cu) for M in (257, 512, 513, 4096))
            continue
        assert thr % 256 == 0 and thr in edges and thr + 1 in edges
        # thr is the last M with 4 * tiles <= n_cu // 8 * 8, thr + 1 the first without
        assert 4 * (thr // 256) * (-(-N // 256)) <= n_cu // 8 * 8 < 4 * (thr // 256 + 1) * (-(-N // 256))
        assert not _mid_usable(thr + 1, N, n_cu)
        if thr > 256:
            assert _mid_usable(thr, N, n_cu)
        else:  # so few CUs that this product never takes the mid kernel: 256 / 257 are in the fixed edges anyway
            assert not _mid_usable(thr, N, n_cu) and thr == 256


@pytest.mark.parametrize("T", [1, 16, 17, 64, 255, 256, 257, 1025, 5377])
def test_builders_return_exactly_what_was_asked(T):
    seqs, which = one_token_batch(T)
    assert len(seqs) == T == len(which) and all(len(s) == 1 for s in seqs)
    assert all(np.array_equal(seqs[i], seqs[which[i]]) for i in range(T))  # the first k are the distinct ones
    assert len({int(s[0]) for s in seqs[:23]}) == min(T, 23)               # ... and really distinct
    s3, w3 = three_token_batch(T)
    assert len(s3) == T == len(w3) and all(len(s) == 3 for s in s3)
    assert all(np.array_equal(s3[i], s3[w3[i]]) for i in range(T))
    assert len({tuple(s.tolist()) for s in s3[:23]}) == min(T, 23)
    if T >= 64:
        assert np.bincount(which).min() >= 2 and np.bincount(w3).min() >= 2
    sr, wr = ragged_batch(T)
    assert sum(len(s) for s in sr) == T and len(sr) == len(wr)
    assert all(1 <= len(s) <= max(RAGGED_LENS) for s in sr)
    assert all(int(s.max()) < 64 and int(s.min()) >= 0 for s in sr)
    first = {}
    for s, j in zip(sr, wr.tolist()):
        assert np.array_equal(first.setdefault(j, s), s)  # equal index, equal tokens
    distinct, dense = distinct_of(sr, wr)
    assert len(distinct) == len(first) and all(np.array_equal(distinct[j], s) for s, j in zip(sr, dense))
    assert len({tuple(s.tolist()) for s in distinct}) == len(distinct)
    if T >= 5377:  # two full cycles of the 23 sequences (1339 tokens each): every one of them repeats
        assert np.bincount(wr)[:23].min() >= 2
        starts = np.concatenate([[0], np.cumsum([len(s) for s in sr])[:-1]])
        for j in range(23):  # ... at another offset inside a 128-row panel
            assert len({int(o) % 128 for o in starts[wr == j]}) >= 2


def _small():
    shape = obert.BertShape(2, 128, 4, 256, vocab=64, max_pos=128)
    return shape, f64_weights(obert.random_weights(shape, 5))


def test_f64_weight_views_change_no_bit_of_the_oracle():
    shape = obert.BertShape(2, 128, 4, 256, vocab=64, max_pos=128)
    w = obert.random_weights(shape, 5)
    seqs = ragged_batch(300)[0][:8]
    for pooling in ("cls", "mean"):
        plain = obert.sentence_embeddings(w, shape, seqs, pooling, True, np.float64)
        assert np.array_equal(plain, obert.sentence_embeddings(f64_weights(w), shape, seqs, pooling, True, np.float64))
    assert all(v.dtype == np.float32 for v in w.values())  # (the caller's weights are left alone)


def test_check_rows_passes_the_oracle_and_sees_other_bits_in_a_repeat():
    shape, w = _small()
    seqs, which = one_token_batch(300)
    want = obert.sentence_embeddings(w, shape, seqs[:23], "mean", True, np.float64)
    got = want[which].astype(np.float32)
    dcos, dabs = check_rows(got, want, which, "f32")
    assert dcos < 1e-6 and dabs < 1e-7
    got[23 * 7 + 4] = np.nextafter(got[23 * 7 + 4], np.float32(2.0))  # one ulp, far inside every tolerance
    with pytest.raises(AssertionError, match="differ in bits"):
        check_rows(got, want, which, "f32")


def test_one_wrong_row_fails_check_rows_and_passes_the_mean_pooled_check():
    """The gap the every-row tests close, on oracle output alone. The same slip, 2e-3 on one component of one token
    row in units of that row's length, is (a) four times TOL['f16'][1] = 5e-4 when the row is its own embedding, and
    (b) divided by the 128 tokens of its sequence before the pooled check of test_encoder_gpu applies the same 5e-4."""
    from test_encoder_gpu import TOL, _check

    slip = 2e-3
    assert slip > 2 * TOL["f16"][1] and slip / 128 < TOL["f16"][1] / 2  # read from TOL: the contrast holds with margin
    shape, w = _small()
    seqs, which = one_token_batch(300)
    want = obert.sentence_embeddings(w, shape, seqs[:23], "mean", True, np.float64)
    got = want[which].astype(np.float32)
    check_rows(got, want, which, "f16")
    got[257, 77] += slip  # the one row past a 256-row tile
    with pytest.raises(AssertionError, match="1 of 300 rows outside"):
        check_rows(got, want, which, "f16")

    ids = np.random.default_rng(7).integers(0, shape.vocab, size=128).astype(np.int32)
    hidden = obert.encode_one(w, shape, ids, np.float64)

    def pooled(h):
        e = h.mean(axis=0)
        return (e / np.linalg.norm(e))[None, :]

    wrong = hidden.copy()
    wrong[127, 77] += slip * np.linalg.norm(hidden[127])  # the same slip relative to the row: the larger reading
    assert np.abs(pooled(wrong) - pooled(hidden)).max() > 0.0
    _check(pooled(wrong), pooled(hidden), "one wrong token row of 128, mean pooled", "f16")
