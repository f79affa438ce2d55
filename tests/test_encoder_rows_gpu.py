"""Every row of every GEMM output of the HIP encoder against the NumPy f64 oracle, at every token count where the
forward pass changes kernel (encoder_rows_case.route_edges). The batches are built so that no row hides behind a
pooling: one-token sequences (a row is its own embedding), three-token sequences under CLS pooling (the [CLS]-only
tail of the last layer at M = n_seq) and ragged sequences with real attention. Distinct sequences are few, so the
oracle is cheap, and every repeat must carry the bits of the first occurrence wherever its rows fall in a tile."""
import time

import numpy as np
import pytest

from encoder_rows_case import (check_rows, distinct_of, f64_weights, one_token_batch, ragged_batch, route_edges,
                               three_token_batch)
from oracle import bert as obert

pytestmark = pytest.mark.gpu
WIDTHS = ["all-MiniLM-L6-v2", "bge-base-en-v1.5", "bge-large-en-v1.5"]  # H = 384, 768, 1024
LAYERS = 3  # a first, a middle and a last layer: EPI_RLS_R32_O16, EPI_RLS_R16_O16, EPI_FOLD_*, EPI_RLS_R16_O32 / f32 rows
VOCAB = 64
F32_EDGES = (127, 128, 129, 255, 256, 257, 384, 385, 1025)


class _Oracle:
    """One width: seeded weights, their f64 copies, and the f64 embedding of every distinct sequence asked for so far."""

    def __init__(self, name):
        base, _ = obert.SHAPES[name]
        self.shape = obert.BertShape(LAYERS, base.hidden, base.heads, base.intermediate, vocab=VOCAB, max_pos=256)
        self.w = obert.random_weights(self.shape, 41)
        self.w64 = f64_weights(self.w)
        self.memo = {}

    def want(self, seqs, pooling):
        rows = []
        for s in seqs:
            key = ("one" if len(s) == 1 else pooling, s.tobytes())  # one token: its [CLS] row is its mean
            if key not in self.memo:
                self.memo[key] = obert.sentence_embeddings(self.w64, self.shape, [s], pooling, True, np.float64)[0]
            rows.append(self.memo[key])
        return np.stack(rows)


@pytest.fixture(scope="module")
def oracles():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Oracle(name)
            made[name].want(one_token_batch(23)[0], "cls")    # the 23 one-token passes per width, once
        return made[name]

    return get


@pytest.fixture(scope="module")
def n_cu(gpu):
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


class _Engine:
    def __init__(self, orc, pooling, precision):
        from voitta_rag_amd import Engine
        from voitta_rag_amd import encoder as enc

        self.enc, s = enc, orc.shape
        self.e = Engine(s.hidden)
        enc.load_encoder(self.e, enc.BertDesc(s.layers, s.hidden, s.heads, s.intermediate, vocab=s.vocab, max_pos=s.max_pos,
                                              pooling=pooling, normalize=True, eps=s.eps, precision=precision), orc.w)

    def encode(self, seqs):
        off = np.zeros(len(seqs) + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in seqs])
        return self.enc.encode(self.e, np.concatenate(seqs).astype(np.int32), off)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.close()


def _run(eng, orc, pooling, precision, batch, what):
    seqs, which = batch
    distinct, which = distinct_of(seqs, which)
    got = eng.encode(seqs)
    dcos, dabs = check_rows(got, orc.want(distinct, pooling), which, precision)
    print(f"{what}: {len(seqs)} rows, worst |1-cos| = {dcos:.3e}, worst abs diff = {dabs:.3e}")
    return got


@pytest.mark.parametrize("pooling", ["cls", "mean"])
@pytest.mark.parametrize("name", WIDTHS)
def test_every_row_at_every_route_edge(gpu, oracles, n_cu, name, pooling):
    """T one-token sequences with n_seq == T: the CLS tail does not engage, so all T rows of all three layers run the
    full-T kernels, and each returned row is one GEMM row. cls and mean give the same numbers here but end the last
    layer differently (EPI_RLS_R16_O16 and statistics only, against EPI_RLS_R16_O32 and the final LayerNorm's f32 rows)."""
    orc, t0 = oracles(name), time.perf_counter()
    with _Engine(orc, pooling, "f16") as eng:
        for T in route_edges(orc.shape.hidden, orc.shape.intermediate, n_cu):
            _run(eng, orc, pooling, "f16", one_token_batch(T), f"{name} {pooling} f16 one-token T={T}")
    print(f"{name} {pooling}: {n_cu} CUs, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("name", WIDTHS)
def test_cls_tail_rows_at_every_route_edge(gpu, oracles, n_cu, name):
    """n three-token sequences, CLS pooling: the last layer's output projection, FFN and LayerNorms run on the n
    gathered [CLS] rows (the same route ladder at M = n), the layers before it at M = 3n."""
    orc, t0 = oracles(name), time.perf_counter()
    with _Engine(orc, "cls", "f16") as eng:
        for n in route_edges(orc.shape.hidden, orc.shape.intermediate, n_cu):
            if n <= 2048:
                _run(eng, orc, "cls", "f16", three_token_batch(n), f"{name} cls f16 CLS tail n_seq={n} T={3 * n}")
    print(f"{name} cls tail: {n_cu} CUs, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("name", WIDTHS)
def test_ragged_rows_at_every_route_edge(gpu, oracles, n_cu, name):
    """Real attention, sequences across the 64-key, 128-row and 256-row edges, mean pooling. Repeats of one sequence
    start at different tile offsets; the mid and the ping-pong kernel are row-independent and bit-identical to each
    other and attention_seq_kernel works per sequence, so the same bits are required."""
    orc, t0 = oracles(name), time.perf_counter()
    with _Engine(orc, "mean", "f16") as eng:
        for T in route_edges(orc.shape.hidden, orc.shape.intermediate, n_cu):
            if T >= 256:
                _run(eng, orc, "mean", "f16", ragged_batch(T), f"{name} mean f16 ragged T={T}")
    print(f"{name} ragged: {n_cu} CUs, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_f32_and_f16x3_rows_at_their_tile_edges(gpu, oracles, n_cu, precision):
    """The other two precisions at their own tile edges. f16x3: N % 256 != 0 at H = 384 keeps the 128-row kernel
    (gemm_f16x3_kernel) at every M, H = 768 switches to the 256-row kernel at M >= 256."""
    t0 = time.perf_counter()
    for name in WIDTHS[:2]:
        orc = oracles(name)
        with _Engine(orc, "mean", precision) as eng:
            for T in F32_EDGES:
                _run(eng, orc, "mean", precision, one_token_batch(T), f"{name} mean {precision} one-token T={T}")
                _run(eng, orc, "mean", precision, ragged_batch(T), f"{name} mean {precision} ragged T={T}")
    print(f"{precision}: {n_cu} CUs, {time.perf_counter() - t0:.2f} s")


def test_replayed_graph_keeps_every_row(gpu, oracles, n_cu):
    """T <= 1024 is captured into a hipGraph the second time a shape is seen: eager, captured and replayed runs of
    one batch agree bit for bit, and the replayed rows hold the every-row bar."""
    orc, t0 = oracles("bge-base-en-v1.5"), time.perf_counter()
    with _Engine(orc, "cls", "f16") as eng:
        for T in (257, 1024):
            batch = one_token_batch(T)
            eager, captured = eng.encode(batch[0]), eng.encode(batch[0])
            replayed = _run(eng, orc, "cls", "f16", batch, f"bge-base cls f16 one-token T={T}, replayed graph")
            assert np.array_equal(eager.view(np.uint32), captured.view(np.uint32))
            assert np.array_equal(eager.view(np.uint32), replayed.view(np.uint32))
    print(f"replay: {n_cu} CUs, {time.perf_counter() - t0:.2f} s")
