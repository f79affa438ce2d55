"""Every token row of the rotary, gated and pre-norm routes of the HIP encoder against the families' NumPy f64 oracles, at
real widths and at every token count where the forward pass changes kernel (encoder_family_rows_case.py): forward_chunk
as nomic (rotary, SwiGLU / GeGLU) and as ALiBi (GeGLU, slopes), forward_chunk_prenorm (ModernBERT), forward_chunk_rms (T5)
and forward_chunk_rms_rotary (Qwen2). Every token of span_batch(T) is returned as a one-token span, so a wrong row of a
rotation, a gate, a norm or a residual hand-over is an output and not 1 / length of one; repeats of a (sequence, token)
must carry the bits of the first occurrence wherever they fall in a tile. test_encoder_family_rows_cpu.py shows, on
oracle output alone, that the mistakes these tests are for would fail them."""
import numpy as np
import pytest

from encoder_family_rows_case import (FAMILIES, FOLD_TOKENS, WIDTHS, Tally, family_route_edges, model, run_pooled,
                                      run_token_rows, span_batch, token_spans)
from encoder_rows_case import FIXED_EDGES, three_token_batch
from test_encoder_rows_gpu import F32_EDGES

pytestmark = pytest.mark.gpu
CASES = [(f, H) for f in FAMILIES for H in WIDTHS] + [("qwen2", 896)]
FOLD_CASES = ([("qwen2", H) for H in (384, 768, 896, 1024)] +
              [(f, H) for f in ("t5", "modernbert", "nomic-silu") for H in (384, 768, 1024)])


@pytest.fixture(scope="module")
def n_cu(gpu):
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("part", ["fixed", "threshold"])
@pytest.mark.parametrize("family,H", CASES)
def test_every_token_row_at_every_route_edge(gpu, n_cu, family, H, part):
    """f16. "fixed": FIXED_EDGES — the folded norms (T <= 16), the skinny kernels' row blocks with the rotation and the
    gate in their epilogues (T <= 256; the split-K pair at H = 896), then rope_kernel / glu_kernel or, post-norm,
    EPI_FOLD_SWIGLU / EPI_FOLD_GEGLU in the mid kernel. "threshold": both sides of mid_threshold(N) for each N of the
    family, the last M on gemm_f16_mid_kernel and the first on gemm_f16_pp_kernel."""
    m, tally = model(family, H), Tally()
    edges = family_route_edges(m.Ns, n_cu)
    e = m.engine("mean", "f16")
    try:
        for T in edges:
            if (T in FIXED_EDGES) == (part == "fixed"):
                run_token_rows(e, m, span_batch(T), "f16", f"every token, T={T}", tally)
    finally:
        e.close()
    tally.report(f"{m.name} {part}", n_cu)


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
@pytest.mark.parametrize("family,H", [(f, H) for f in FAMILIES for H in WIDTHS])
def test_f32_and_f16x3_token_rows_at_their_tile_edges(gpu, n_cu, family, H, precision):
    """The unfused twins at every M: rope_kernel<float>, glu_kernel<float, 1 | 0>, rmsnorm_kernel at both widths."""
    m, tally = model(family, H), Tally()
    e = m.engine("mean", precision)
    try:
        for T in F32_EDGES:
            run_token_rows(e, m, span_batch(T), precision, f"every token, T={T}", tally)
    finally:
        e.close()
    tally.report(f"{m.name} {precision}", n_cu)


@pytest.mark.parametrize("family,H", FOLD_CASES)
def test_folded_norm_question_route(gpu, n_cu, family, H):
    """One sequence of 1, 9, 16 and 17 tokens, f16, all rows exposed: up to 16 rows run the projections with the norm
    folded in (gemm_f16_skinny_ln_rope_kernel, gemm_f16_skinny_rms_kernel, gemm_f16_skinny_rms_rope_kernel; K = 896 is
    Qwen2's alone), 17 the norm launches. Three runs, bit-identical: the second is captured, the third replayed."""
    from voitta_rag_amd import encoder as enc

    m, tally = model(family, H), Tally()
    e = m.engine("mean", "f16")
    try:
        for n in FOLD_TOKENS:
            seq = np.random.default_rng(400 + n).integers(0, m.shape.vocab, size=n).astype(np.int32)
            batch = ([seq], np.zeros(1, np.int64))
            first = run_token_rows(e, m, batch, "f16", f"one sequence of {n}", tally)
            for _ in range(2):
                assert np.array_equal(_bits(first), _bits(enc.encode_spans(e, *token_spans([seq])))), n
    finally:
        e.close()
    tally.report(f"{m.name} folded", n_cu)


@pytest.mark.parametrize("family,H", [(f, H) for f in ("nomic-silu", "nomic-gelu", "alibi") for H in WIDTHS])
def test_cls_tail_with_a_gate(gpu, n_cu, family, H):
    """n three-token sequences under CLS pooling through encode: the last layer's FFN runs on the n gathered [CLS] rows,
    its gate fused by fuse_glu(n_seq) while the body's goes by fuse_glu(T = 3n) — on both sides of every edge."""
    m, tally = model(family, H), Tally()
    e = m.engine("cls", "f16")
    try:
        for n in family_route_edges(m.Ns, n_cu):
            if n <= 2048:
                run_pooled(e, m, three_token_batch(n), "cls", "f16", f"CLS tail, n_seq={n}, T={3 * n}", tally)
    finally:
        e.close()
    tally.report(f"{m.name} cls tail", n_cu)


@pytest.mark.parametrize("family,H", [(f, H) for f in FAMILIES for H in WIDTHS])
def test_pooled_rows(gpu, n_cu, family, H):
    """encode with mean, cls and (Qwen2: VR_POOL_LAST) last pooling on span_batch(257) and span_batch(1025)."""
    m, tally = model(family, H), Tally()
    for pooling in ("mean", "cls") + (("last",) if family == "qwen2" else ()):
        e = m.engine(pooling, "f16")
        try:
            for T in (257, 1025):
                run_pooled(e, m, span_batch(T), pooling, "f16", f"T={T}", tally)
        finally:
            e.close()
    tally.report(f"{m.name} pooled", n_cu)


@pytest.mark.parametrize("family", FAMILIES)
def test_replayed_graph_keeps_every_token_row(gpu, n_cu, family):
    """T <= 1024 is captured the second time a shape is seen: eager, captured and replayed runs agree bit for bit."""
    from voitta_rag_amd import encoder as enc

    m, tally = model(family, 768), Tally()
    e = m.engine("mean", "f16")
    try:
        for T in (257, 1024):
            batch = span_batch(T)
            arrays = token_spans(batch[0])
            eager, captured = enc.encode_spans(e, *arrays), enc.encode_spans(e, *arrays)
            replayed = run_token_rows(e, m, batch, "f16", f"every token, T={T}, replayed graph", tally)
            assert np.array_equal(_bits(eager), _bits(captured)) and np.array_equal(_bits(eager), _bits(replayed)), T
    finally:
        e.close()
    tally.report(f"{m.name} replay", n_cu)
