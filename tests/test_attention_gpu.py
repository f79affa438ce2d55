"""The three attention kernels (attention_kernel: f32 and f16x3; attention_seq_kernel and attention_stream_kernel: f16) in
their five mask / bias states at head sizes 64 and 32, and in the two states head size 128 has (none and causal: the
Qwen3 body, its own swizzle, staging round and LDS opt-ins), through load_encoder, set_attention_bias,
set_attention_slopes, encode and encode_spans alone, on the models of attention_case.py in which one attention layer IS the token row: every query row
of every length that crosses a kernel's edge against the f64 oracle at test_encoder_gpu.TOL. test_attention_cpu.py proves
that each of the catalogue's mistakes would move a row of every query tile it touches by more than twice that bar."""
import numpy as np
import pytest

import attention_case as ac
from test_encoder_gpu import TOL

pytestmark = pytest.mark.gpu
MODELS = ac.PAIRS  # every (state, head size) launch_attention has an instantiation for


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def kernel_of(m, precision, param, max_len):
    """The kernel launch_attention picks for a pass whose longest sequence has max_len tokens."""
    if precision != "f16":
        return "attention_kernel"
    table = 4 * (2 * param + 1) if m.state == "table" and param else 0
    staged = 4 * ((max_len + 15) & ~15) * m.dh + table <= 160 * 1024  # 2 (K, V) * 2 bytes * lds_keys * d_h + the table's
    if m.state == "window" and param and max_len >= 384:  # kWindowStreamFrom
        staged = False
    return "attention_seq_kernel" if staged else "attention_stream_kernel"


WORST = {}


def check(got, want, precision, what, kernel=None):
    """Every row within TOL[precision] of the oracle's, cosine and absolute; the worst of both is kept per `kernel`."""
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), what
    dcos, dabs = ac.deviation(got, want)
    if kernel:
        old = WORST.get(kernel, (0.0, 0.0))
        WORST[kernel] = (max(old[0], float(dcos.max())), max(old[1], float(dabs.max())))
    cos_tol, abs_tol = TOL[precision]
    bad = np.flatnonzero(~((dcos < cos_tol) & (dabs < abs_tol)))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(got)} rows outside TOL[{precision}], rows {bad[:16].tolist()}, "
                           f"worst |1-cos| {dcos.max():.3e}, worst abs {dabs.max():.3e}")


def report(m, precision):
    for kernel, (c, a) in sorted(WORST.items()):
        print(f"ATTENTION {m.name} {precision} {kernel}: worst |1-cos| {c:.3e}, worst abs {a:.3e}")
    WORST.clear()


def engines(m, precision, params, pooling="mean"):
    """(param, engine) for each parameter value: a window is part of the description (an engine each), a table is set on
    the one engine."""
    if m.state == "window":
        for param in params:
            e = m.engine(precision, pooling, param)
            yield param, e
            e.close()
        return
    e = m.engine(precision, pooling)
    for param in params:
        m.set_param(e, param)
        yield param, e
    e.close()


# ---- 1. every row of every length ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", list(TOL))
@pytest.mark.parametrize("state, dh", MODELS)
def test_every_row_against_the_oracle(gpu, state, dh, precision):
    m = ac.model(state, dh)
    cases = ac.cases(state, dh, precision)
    params = list(dict.fromkeys(p for p, _ in cases))
    for param, e in engines(m, precision, params):
        for S in [s for p, s in cases if p == param]:
            got = ac.token_rows(e, [ac.sequence(S)])
            check(got, m.rows(S, param), precision, f"{m.name} param {param} S {S}", kernel_of(m, precision, param, S))
    report(m, precision)


# ---- 2. batch composition ------------------------------------------------------------------------------------------------
def _param(m):
    return {"window": 64, "table": 64}.get(m.state)


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("state, dh", MODELS)
def test_a_sequence_beside_others(gpu, state, dh, precision):
    """max_len sizes lds_keys, qblocks and the kernel choice of the whole launch: a 129-token sequence alone, beside a
    shorter one and a longer one (f16: one that takes the launch to the streamed kernel), and twice in one batch (the same
    bits in both places)."""
    m, param = ac.model(state, dh), _param(ac.model(state, dh))
    longer = 193 if precision != "f16" else ac.STREAMED[dh][0]
    a, short, long_ = ac.sequence(129), ac.sequence(17), ac.sequence(longer)
    for _, e in engines(m, precision, [param]):
        for name, batch in (("alone", [a]), ("beside a shorter", [short, a]), ("twice, beside both", [short, a, long_, a])):
            got = ac.token_rows(e, batch)
            want = np.concatenate([m.rows(len(s), param) for s in batch])
            check(got, want, precision, f"{m.name} {name}", kernel_of(m, precision, param, max(len(s) for s in batch)))
        first, second = got[17:17 + 129], got[17 + 129 + longer:]
        assert np.array_equal(_bits(first), _bits(second))
    report(m, precision)


@pytest.mark.parametrize("state, dh, precision", [("none", 64, "f16"), ("causal", 32, "f16"), ("causal", 128, "f16"),
                                                  ("table", 64, "f16"),
                                                  ("slopes", 32, "f32"), ("window", 64, "f32")])
def test_a_batch_that_forward_all_splits(gpu, state, dh, precision):
    """More than kMaxChunkTokens = 262144 tokens: the second chunk's launches run with seq0 and tok_base behind the first.
    Three distinct sequences repeat; every repeat carries the bits of the first occurrence, which is held to the oracle."""
    m, param = ac.model(state, dh), _param(ac.model(state, dh))
    distinct = [ac.sequence(257), ac.sequence(129), ac.sequence(65)]
    per = sum(len(s) for s in distinct)
    n = ac.KERNEL_SPLIT // per + 32  # 32 repeats of the three behind the split
    assert (n - 32) * per <= ac.KERNEL_SPLIT < (n - 31) * per
    for _, e in engines(m, precision, [param]):
        got = ac.token_rows(e, distinct * n).reshape(n, per, ac.H)
        want = np.concatenate([m.rows(len(s), param) for s in distinct])
        check(got[0], want, precision, f"{m.name} first occurrence", kernel_of(m, precision, param, 257))
        differ = np.flatnonzero((_bits(got) != _bits(got[0])[None]).any(axis=(1, 2)))
        assert differ.size == 0, f"repeats {differ[:8].tolist()} of {n} differ in bits from the first"
    report(m, precision)


# ---- 3. the CLS tail -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("state, dh", MODELS)
def test_cls_pooling_is_the_first_tokens_row(gpu, state, dh, precision):
    """Under CLS pooling the last layer's attention is the q_limit = 16 launch (one query tile or block per sequence):
    encode's row equals the oracle's row of token 0, and the row of span (0, 1), at lengths on both sides of 16, 64 and
    128 and (f16) on the streamed route — each alone and all in one batch."""
    from voitta_rag_amd import encoder as enc

    m, param = ac.model(state, dh), _param(ac.model(state, dh))
    lens = [15, 16, 17, 63, 64, 65, 127, 128, 129] + ([ac.STREAMED[dh][0]] if precision == "f16" else [])
    seqs = [ac.sequence(S) for S in lens]
    want = np.stack([m.rows(S, param)[0] for S in lens])
    for _, e in engines(m, precision, [param], pooling="cls"):
        for i, s in enumerate(seqs):
            got = enc.encode(e, *ac.pack([s]))
            check(got, want[i:i + 1], precision, f"{m.name} CLS of {lens[i]} tokens", kernel_of(m, precision, param, lens[i]))
            ids, off = ac.pack([s])
            span = enc.encode_spans(e, ids, off, np.array([0, 1], np.int32), np.array([[0, 1]], np.int32))
            check(span, got.astype(np.float64), precision, f"{m.name} span (0, 1) of {lens[i]} tokens")
        check(enc.encode(e, *ac.pack(seqs)), want, precision, f"{m.name} CLS, one batch", kernel_of(m, precision, param, lens[-1]))
    report(m, precision)


# ---- 4. graph replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("state, dh", MODELS)
def test_replayed_calls_give_the_first_calls_bits(gpu, state, dh, precision):
    """forward_all captures a shape of at most 1024 tokens the second time it sees it and replays the graph from the third
    call on: three calls of one shape, the same bits."""
    m, param = ac.model(state, dh), _param(ac.model(state, dh))
    # (f16: a streamed length where one of at most 1024 tokens exists — d_h = 32 streams from 1281 on)
    lens = (129, 257) if precision != "f16" else (129, {64: 641, 32: 1024, 128: 449}[dh])
    for _, e in engines(m, precision, [param]):
        for S in lens:
            runs = [ac.token_rows(e, [ac.sequence(S)]) for _ in range(3)]
            check(runs[0], m.rows(S, param), precision, f"{m.name} S {S}", kernel_of(m, precision, param, S))
            assert np.array_equal(_bits(runs[0]), _bits(runs[1])) and np.array_equal(_bits(runs[0]), _bits(runs[2])), S
    report(m, precision)


# ---- 5. state changes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("state, dh", [(s, d) for s, d in MODELS if s in ("table", "slopes")])
def test_setting_removing_and_resetting_the_bias(gpu, state, dh, precision):
    m = ac.model(state, dh)
    on, other, off = (64, 5, None) if state == "table" else ("on", None, "off")
    S = 129
    seq = ac.sequence(S)
    e = m.engine(precision)
    rows = {}
    for step, param in enumerate((on, off, other, on, off) if other else (on, off, on, off)):
        m.set_param(e, param)
        got = ac.token_rows(e, [seq])
        check(got, m.rows(S, param), precision, f"{m.name} step {step} param {param}", kernel_of(m, precision, param, S))
        if param in rows:
            assert np.array_equal(_bits(got), _bits(rows[param])), (step, param)
        rows[param] = got
    assert not np.array_equal(rows[on], rows[off])
    e.close()
    report(m, precision)


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("dh", ac.HEAD_SIZES)
def test_window_zero_is_the_global_model(gpu, dh, precision):
    m = ac.model("window", dh)
    e = m.engine(precision, param=0)
    for S in (129, 449):
        got = ac.token_rows(e, [ac.sequence(S)])
        check(got, m.rows(S, 0), precision, f"{m.name} window 0 S {S}", kernel_of(m, precision, 0, S))
        assert np.max(np.abs(m.rows(S, 0) - m.rows(S, 64))) > 50 * TOL[precision][1]  # the two models are far apart
    e.close()
    report(m, precision)
