"""The last layer of a [CLS]-pooled f16 model attended from the [CLS] rows on the hidden rows themselves (`collapse` in
csrc/encoder.hip's forward_chunk: cls_head_gemm_kernel, cls_attend_kernel) against the f64 oracle, on the inputs that
test_cls_collapse_cpu.py proves sensitive: a kernel that makes one of cls_collapse_case.MISTAKES fails the parity test.
Then what must hold around it: a sequence's bits do not depend on its place, graphs replay the same bits, every route
outside the guard is untouched by the switch, and the route is really taken where it should be."""
import os

import numpy as np
import pytest

import cls_collapse_case as cc
from oracle import bert as obert
from test_encoder_gpu import TOL

pytestmark = pytest.mark.gpu


def _both(shape, w, seqs, **kw):
    """The same batch through an engine with the route and one loaded under VR_CLS_COLLAPSE=0."""
    out = []
    for collapse in (True, False):
        e = cc.engine(shape, w, collapse=collapse, **kw)
        out.append(cc.encode(e, seqs))
        e.close()
    return out


def _parity(name, shape, w, seqs, want):
    on, off = _both(shape, w, seqs)
    dcos, dabs = cc.deviation(on, want)
    ocos, oabs = cc.deviation(on, off.astype(np.float64))
    print(f"{name}: {sum(len(s) for s in seqs)} tokens, worst |1-cos| {dcos.max():.3e}, worst abs diff {dabs.max():.3e}; "
          f"from a VR_CLS_COLLAPSE=0 engine |1-cos| {ocos.max():.3e}, abs {oabs.max():.3e}")
    assert np.all(np.isfinite(on))
    assert dcos.max() < TOL["f16"][0] and dabs.max() < TOL["f16"][1]


@pytest.mark.parametrize("dh", cc.HEAD_SIZES)
def test_dominant_attention_models_against_the_f64_oracle(gpu, dh):
    m = cc.model(dh)
    seqs = cc.ladder_batch()
    assert sum(len(s) for s in seqs) > 256
    _parity(m.name, m.shape, m.w, seqs, m.oracle_rows(seqs))


@pytest.mark.parametrize("hidden,heads,layers", [(384, 12, 2), (384, 12, 3), (768, 12, 2), (768, 12, 3)])
def test_ordinary_models_against_the_f64_oracle(gpu, hidden, heads, layers):
    shape = obert.BertShape(layers, hidden, heads, 4 * hidden, vocab=cc.VOCAB, max_pos=cc.MAX_POS)
    w = obert.random_weights(shape, 41)
    seqs = cc.ladder_batch()
    want = obert.sentence_embeddings(w, shape, seqs, "cls", True, np.float64)
    _parity(f"H{hidden} x{heads} L{layers}", shape, w, seqs, want)


def test_a_sequence_does_not_depend_on_its_place(gpu):
    """A batch and a copy rotated by an odd number of sequences agree bit for bit; so does a batch beyond 262144 tokens,
    where a second forward chunk starts (seq0, tok_base > 0)."""
    for dh in cc.HEAD_SIZES:
        m = cc.model(dh)
        seqs = cc.ladder_batch()
        e = cc.engine(m.shape, m.w)
        here = cc.encode(e, seqs)
        there = cc.encode(e, seqs[7:] + seqs[:7])
        assert np.array_equal(np.concatenate([there[-7:], there[:-7]]), here)
        e.close()
    m = cc.model(32)
    rng = np.random.default_rng(8)
    lens = rng.integers(1, cc.MAX_POS + 1, size=2200).tolist()
    seqs = [cc.sequence(n, i) for i, n in enumerate(lens)]
    assert sum(lens) > cc.KERNEL_SPLIT
    e = cc.engine(m.shape, m.w)
    here = cc.encode(e, seqs)
    there = cc.encode(e, seqs[777:] + seqs[:777])
    e.close()
    assert np.all(np.isfinite(here))
    assert np.array_equal(np.concatenate([there[-777:], there[:-777]]), here)


def test_eager_captured_and_replayed_runs_agree(gpu):
    """Between 257 and 1024 tokens a shape is captured into a hipGraph the second time it is seen: no allocation and no
    host wait on the route."""
    m = cc.model(64)
    seqs = [cc.sequence(S, i) for i, S in enumerate((129, 64, 33, 17, 257, 1, 100))]
    assert 256 < sum(len(s) for s in seqs) <= 1024
    e = cc.engine(m.shape, m.w)
    eager, captured, replayed = cc.encode(e, seqs), cc.encode(e, seqs), cc.encode(e, seqs)
    e.close()
    assert np.array_equal(eager, captured) and np.array_equal(eager, replayed)
    dcos, dabs = cc.deviation(eager, m.oracle_rows(seqs))
    assert dcos.max() < TOL["f16"][0] and dabs.max() < TOL["f16"][1]


def _same_bits(shape, w, seqs, **kw):
    on, off = _both(shape, w, seqs, **kw)
    assert np.all(np.isfinite(on)) and np.array_equal(on, off)


def test_routes_outside_the_guard_do_not_move(gpu):
    """Bit for bit the same with and without the switch: whatever the guard of `collapse` excludes."""
    m = cc.model(64)
    seqs = cc.ladder_batch()
    _same_bits(m.shape, m.w, seqs, pooling="mean")
    _same_bits(m.shape, m.w, seqs, precision="f32")
    _same_bits(m.shape, m.w, seqs, precision="f16x3")
    _same_bits(m.shape, m.w, [cc.sequence(S) for S in (100, 64, 33, 17, 1)])  # at most 256 tokens: no folded LayerNorm
    one = obert.BertShape(1, cc.H, 2, cc.I, vocab=cc.VOCAB, max_pos=cc.MAX_POS)
    _same_bits(one, obert.random_weights(one, 5), seqs)
    # beyond the bounds of the guard: more than kClsHeads heads; a longest sequence whose logits do not fit the LDS
    # (cls_attend_lds: 672 keys at H = 128); T / n_seq too small for the workspace behind the tail's
    # (the head size cannot leave {32, 64} in this routine: only the Qwen3 form reaches 128)
    wide = obert.BertShape(2, 640, 20, 640, vocab=cc.VOCAB, max_pos=cc.MAX_POS)
    _same_bits(wide, obert.random_weights(wide, 6), seqs)
    long = obert.BertShape(2, cc.H, 2, cc.I, vocab=cc.VOCAB, max_pos=800)
    _same_bits(long, obert.random_weights(long, 7), [cc.sequence(700), cc.sequence(64, 1)])
    _same_bits(m.shape, m.w, [cc.sequence(2, i) for i in range(300)])  # (the [CLS] tail itself still fits)
    # spans of a CLS model pool as a mean-pooled model's do
    from voitta_rag_amd import encoder as enc

    ids, off = cc.pack(seqs[:6])
    spans = np.asarray([[0, len(s)] for s in seqs[:6]], np.int32)
    rows = []
    for collapse in (True, False):
        e = cc.engine(m.shape, m.w, collapse=collapse)
        rows.append(enc.encode_spans(e, ids, off, np.arange(7, dtype=np.int32), spans))
        e.close()
    assert np.array_equal(rows[0], rows[1])


def _switched(collapse, make):
    before = os.environ.get("VR_CLS_COLLAPSE")
    os.environ["VR_CLS_COLLAPSE"] = "1" if collapse else "0"
    try:
        return make()
    finally:
        if before is None:
            del os.environ["VR_CLS_COLLAPSE"]
        else:
            os.environ["VR_CLS_COLLAPSE"] = before


def test_alibi_and_rotary_cls_models_do_not_move(gpu):
    import alibi_oracle as ao
    import rope_oracle as ro
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    seqs = [np.random.default_rng(i).integers(0, 300, size=n).astype(np.int32) for i, n in enumerate((129, 64, 100, 17, 33))]
    ids, off = cc.pack(seqs)
    ashape = ao.AlibiShape(2, cc.H, 2, cc.I, vocab=300)
    aw = ao.random_weights(ashape, 3)
    rshape = ro.RopeShape(2, cc.H, 2, cc.I, vocab=300, max_pos=256)
    rw = ro.random_weights(rshape, 4)
    slopes = np.asarray([0.5, 0.1], np.float32)
    for desc, w in ((ao.desc_for(ashape, "cls", "f16", max_pos=256, attention_slopes=slopes), aw),
                    (ro.desc_for(rshape, "cls", "f16"), rw)):
        got = []
        for collapse in (True, False):
            def make():
                e = Engine(cc.H)
                enc.load_encoder(e, desc, w)
                return e
            e = _switched(collapse, make)
            got.append(enc.encode(e, ids, off))
            e.close()
        assert np.all(np.isfinite(got[0])) and np.array_equal(got[0], got[1])


def test_the_route_is_taken_on_the_bench_shape_family(gpu):
    """3 layers, CLS pooling, 600 tokens at the bench's width: the profiler counts one Q/K/V projection of the T rows
    fewer and the route's three small products in its place (the [CLS] queries, u, the context rows), the same number of
    attention launches, and the FLOP of both classes say which kernels ran."""
    hidden, heads = 768, 12
    shape = obert.BertShape(3, hidden, heads, 4 * hidden, vocab=cc.VOCAB, max_pos=cc.MAX_POS)
    w = obert.random_weights(shape, 43)
    lens = (120, 97, 64, 33, 128, 101, 57)
    seqs = [cc.sequence(n, i) for i, n in enumerate(lens)]
    T, n = sum(lens), len(lens)
    assert T == 600
    prof = []
    for collapse in (True, False):
        e = cc.engine(shape, w, collapse=collapse)
        e.profile(True)
        cc.encode(e, seqs)
        prof.append((e.profile_read(e.PROF_GEMM), e.profile_read(e.PROF_ATTENTION)))
        e.profile(False)
        e.close()
    (g_on, a_on), (g_off, a_off) = prof
    print(f"GEMM launches {g_on[1]} / {g_off[1]}, attention launches {a_on[1]} / {a_off[1]}")
    assert g_on[1] == g_off[1] - 1 + 3
    assert a_on[1] == a_off[1] == shape.layers
    H = hidden
    removed = 2.0 * T * 3 * H * H
    added = 2.0 * n * H * H + 2 * (2.0 * n * H * H)  # the [CLS] queries; per head [n, dh] x [dh, H] and [n, H] x [H, dh]
    assert g_off[2] - g_on[2] == pytest.approx(removed - added, rel=1e-9)
    qblocks = (max(lens) + 63) // 64
    attn_full = a_off[2] / (shape.layers - 1 + 1.0 / qblocks)  # the old tail books one query block of qblocks
    assert a_on[2] == pytest.approx(attn_full * (shape.layers - 1) + 4.0 * heads * H * T, rel=1e-9)
