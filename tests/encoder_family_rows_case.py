"""TEST INFRASTRUCTURE shared by test_encoder_family_rows_cpu.py and test_encoder_family_rows_gpu.py: the every-row
suite of encoder_rows_case.py for the families that plain BERT does not run — the rotary and gated post-norm forms of
forward_chunk (nomic, ALiBi), forward_chunk_prenorm (ModernBERT), forward_chunk_rms (T5) and forward_chunk_rms_rotary
(Qwen2) — at real widths (H = 384, 768; Qwen2 also 896; 1024 for the folded norms).

One-token sequences are not enough here: position 0 rotates by the identity, one key makes attention trivial and a
causal row 0 sees only itself. span_batch(T) packs exactly T tokens of real sequences, and every token is returned as a
one-token span (encode_spans with n_spans = T), so that every row of every GEMM, rotation, gate and norm of the last
layer is an output, at a position other than zero. The f64 oracle runs once per distinct sequence; every repeat of a
(sequence, token) must also carry the bits of its first occurrence, wherever it falls in a tile.

MISTAKES is the catalogue of deliberate mistakes, planted in the oracles only (their hooks= keyword, or changed
weights), with which test_encoder_family_rows_cpu.py shows that a wrong kernel would move an exposed row past the bar.

NOT in the catalogue, because no output can show them: rotary attention depends on q . k of rotated vectors, which is a
function of the DIFFERENCE of the two positions only. Every position of a sequence shifted by one constant, and
positions that do not restart at a sequence's first token (another constant per sequence), change no logit and no
row. Nobody should count those two slips as covered by this suite; only a mistake that moves a key against its query
("keys of rows >= 16 take the next row's position" below) or changes the angle's scale is visible."""
import functools
import time

import numpy as np

import alibi_oracle as ao
import modernbert_oracle as mo
import qwen2_oracle as qo
import rope_oracle as ro
import t5_oracle as t5
from encoder_rows_case import FIXED_EDGES, _AsIs, distinct_of, f64_weights, mid_threshold
from oracle import bert as obert

LAYERS = 3   # a first, a middle and a last layer
VOCAB = 64
MAX_POS = 256
SPAN_LENS = (2, 17, 63, 64, 65, 129, 1)
FAMILIES = ("nomic-silu", "nomic-gelu", "alibi", "modernbert", "t5", "qwen2")
WIDTHS = (384, 768)
FOLD_TOKENS = (1, 9, 16, 17)


# ---- routes ----------------------------------------------------------------------------------------------------------------
def skinny_slice(K):
    """skinny_slice of csrc/encoder.hip: the split-K slice of the two-launch skinny route."""
    return next((c for c in (192, 256, 128, 64, 32) if K % c == 0), 0)


def skinny_route(M, N, K):
    """skinny_routed of csrc/encoder.hip, with the kernel it names: "one" (gemm_f16_skinny1_kernel: the wave's step count
    admits an unroll of 6, 4 or 3), "split" (gemm_f16_skinny_kernel and skinny_epilogue_kernel) or None (M > 256, or no
    skinny kernel for the shape)."""
    waves = 8 if K % 256 == 0 else 4 if K % 128 == 0 else 0
    steps = K // (32 * waves) if waves else 0
    if M > 256:
        return None
    if steps > 0 and (steps % 6 == 0 or steps % 4 == 0 or steps % 3 == 0) and N % 16 == 0:
        return "one"
    return "split" if skinny_slice(K) > 0 and N % 64 == 0 else None


def family_route_edges(Ns, n_cu):
    """encoder_rows_case.route_edges for a family's own list of output widths Ns — (H, 3H, 4H) for a gated model with
    I = 2H, (H, 3H, I) for T5: FIXED_EDGES and both sides of mid_threshold(N, n_cu) for every N (see route_edges for what
    each number restates)."""
    edges = set(FIXED_EDGES)
    for N in Ns:
        thr = mid_threshold(N, n_cu)
        if thr > 0:
            edges.update((thr, thr + 1))
    return sorted(edges)


# ---- batches ---------------------------------------------------------------------------------------------------------------
def span_batch(T, k=11, vocab=VOCAB):
    """Exactly T tokens, encoder_rows_case.ragged_batch's scheme: k distinct sequences with lengths cycling through
    SPAN_LENS, repeated in order while the next one still fits, then closed with one further distinct sequence (index k)
    of the exact remaining length. One cycle is 487 tokens, no multiple of 128: repeats of a sequence start at different
    offsets inside the 128- and 256-row tiles. Returns (sequences, index of the distinct sequence of each)."""
    rng = np.random.default_rng(203)
    base = [rng.integers(0, vocab, size=SPAN_LENS[j % len(SPAN_LENS)]).astype(np.int32) for j in range(k)]
    closing = rng.integers(0, vocab, size=max(SPAN_LENS)).astype(np.int32)
    seqs, which, total, i = [], [], 0, 0
    while total + len(base[i % k]) <= T:
        seqs.append(base[i % k])
        which.append(i % k)
        total += len(base[i % k])
        i += 1
    if total < T:
        seqs.append(closing[:T - total])
        which.append(k)
    return seqs, np.asarray(which)


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.int32), off


def token_spans(seqs):
    """encode_spans' four arrays with every token a span of its own: (ids, offsets, span_off, span_tok), n_spans = T."""
    ids, off = pack(seqs)
    tok = np.concatenate([np.arange(len(s), dtype=np.int32) for s in seqs])
    return ids, off, off.copy(), np.stack([tok, tok + 1], axis=1).astype(np.int32)


def token_index(seqs, which):
    """(distinct sequences, row) — row[i] for span i of token_spans(seqs): the index of its (distinct sequence, token) in
    the concatenation of the distinct sequences' tokens. Equal row, equal expectation, equal bits."""
    distinct, dense = distinct_of(seqs, which)
    start = np.concatenate([[0], np.cumsum([len(s) for s in distinct])])
    return distinct, np.concatenate([start[j] + np.arange(len(distinct[j])) for j in dense])


def unit(rows):
    return rows / np.linalg.norm(rows, axis=-1, keepdims=True)


def pooled(hidden, pooling):
    x = {"last": lambda: hidden[-1], "mean": lambda: hidden.mean(axis=0), "cls": lambda: hidden[0]}[pooling]()
    return x / np.linalg.norm(x)


def movement(a, b):
    """Per row of two [S, H] hidden states, as check_rows measures: (|1 - cos|, largest |difference| of the unit rows)."""
    ua, ub = unit(a), unit(b)
    return np.abs(1.0 - (ua * ub).sum(axis=1)), np.abs(ua - ub).max(axis=1)


# ---- models ----------------------------------------------------------------------------------------------------------------
class Model:
    """One family at one width: 3 layers, head size 64, I = 2H, vocabulary 64, the family oracle's own seeded weights (cast
    to f64 once) and the f64 hidden states of every sequence asked for so far (computed once, read-only)."""

    def __init__(self, family, H, heads=None, inter=None):
        self.family, self.H = family, H
        heads, I = heads or H // 64, inter or 2 * H
        self.gated = family != "t5"
        self.rotary = family in ("nomic-silu", "nomic-gelu", "modernbert", "qwen2")
        self.prenorm = family in ("modernbert", "t5", "qwen2")
        self.rms = family in ("t5", "qwen2")
        self.act = None if family == "t5" else "silu" if family in ("nomic-silu", "qwen2") else "gelu"
        seed = 300 + 10 * FAMILIES.index(family) + H // 128
        if family.startswith("nomic"):
            self.shape = ro.RopeShape(LAYERS, H, heads, I, vocab=VOCAB, max_pos=MAX_POS, act=self.act)
            self.w = ro.random_weights(self.shape, seed)
        elif family == "alibi":
            from voitta_rag_amd.encoder import alibi_slopes

            self.shape = ao.AlibiShape(LAYERS, H, heads, I, vocab=VOCAB, max_pos=MAX_POS)
            self.w = ao.random_weights(self.shape, seed)
            self.slopes = alibi_slopes(heads)
        elif family == "modernbert":
            self.shape = mo.ModernShape(LAYERS, H, heads, I, vocab=VOCAB, max_pos=MAX_POS, window=64, global_every=2)
            self.w = mo.random_weights(self.shape, seed)
        elif family == "t5":
            self.shape = t5.T5Shape(LAYERS, H, heads, I, vocab=VOCAB)
            self.w = t5.random_weights(self.shape, seed)
        else:
            self.shape = qo.Qwen2Shape(LAYERS, H, heads, 2, I, vocab=VOCAB)
            self.w = qo.random_weights(self.shape, seed)
        # every projection matrix holds f16 values, as attention_case.Model's do: an f16-operand product reads them as
        # they are, which takes the weights' own rounding out of the f16 noise that the CPU tier bounds
        self.w = {k: v.astype(np.float16).astype(np.float32) if v.ndim == 2 and ("layer" in k or "block" in k)
                  and "relative_attention_bias" not in k else v for k, v in self.w.items()}
        self.I = I
        self.N1 = 2 * I if self.gated else I
        self.Ns = (H, 3 * H, self.N1)  # the output widths of the body's products
        self.w64 = f64_weights(self.w)
        self._hidden = {}

    @property
    def name(self):
        return f"{self.family}-{self.H}"

    def theta(self, layer):
        s = self.shape
        return s.theta_local if self.family == "modernbert" and not mo.is_global(s, layer) else s.theta

    def hidden(self, seq, operand=None, hooks=None, w=None):
        """The oracle's final hidden states [S, H] of one sequence, f64; w: other weights (a planted mistake)."""
        w, s = self.w64 if w is None else w, self.shape
        if self.family.startswith("nomic"):
            return ro.encode_one(w, s, seq, operand=operand, hooks=hooks)
        if self.family == "alibi":
            return ao.encode_one(w, s, seq, self.slopes, operand=operand, hooks=hooks)
        if self.family == "modernbert":
            return mo.encode_one(w, s, seq, operand=operand, round_p=True, hooks=hooks)
        if self.family == "t5":
            return t5.encode_one(w, s, seq, operand=operand, hooks=hooks)
        return qo.encode_one(w, s, seq, operand=operand, hooks=hooks)

    def states(self, seq):
        key = np.asarray(seq, np.int32).tobytes()
        if key not in self._hidden:
            self._hidden[key] = self.hidden(seq)
            self._hidden[key].setflags(write=False)
        return self._hidden[key]

    def token_rows(self, distinct):
        """The unit-length rows of every token of the distinct sequences, concatenated (token_index's numbering)."""
        return np.concatenate([unit(self.states(s)) for s in distinct])

    def pooled_rows(self, distinct, pooling):
        return np.stack([pooled(self.states(s), pooling) for s in distinct])

    def desc(self, pooling, precision):
        s = self.shape
        if self.family.startswith("nomic"):
            return ro.desc_for(s, pooling, precision)
        if self.family == "alibi":
            return ao.desc_for(s, pooling, precision, attention_slopes=self.slopes)
        if self.family == "modernbert":
            return mo.desc_for(s, pooling, precision)
        if self.family == "t5":
            return t5.desc_for(s, pooling, precision, max_pos=MAX_POS)
        return qo.desc_for(s, pooling, precision, max_pos=MAX_POS)

    def engine(self, pooling, precision):
        from voitta_rag_amd import Engine
        from voitta_rag_amd import encoder as enc

        e = Engine(self.H)
        enc.load_encoder(e, self.desc(pooling, precision), self.w)
        return e


@functools.lru_cache(maxsize=None)
def model(family, H):
    """The one Model of a family and width in this process: the CPU and the GPU tests share its oracle rows. Qwen2 at 896
    is the 0.5B body's row geometry (14 heads over 2 KV heads) with I = 1792."""
    return Model(family, H, 14, 1792) if H == 896 else Model(family, H)


# ---- what the GPU tests run ------------------------------------------------------------------------------------------------
class Tally:
    """Worst figures over the batches of one test, and the line that reports them."""

    def __init__(self):
        self.t0, self.batches, self.rows, self.dcos, self.dabs = time.perf_counter(), 0, 0, 0.0, 0.0

    def add(self, rows, dcos, dabs):
        self.batches, self.rows = self.batches + 1, self.rows + rows
        self.dcos, self.dabs = max(self.dcos, dcos), max(self.dabs, dabs)

    def report(self, what, n_cu):
        print(f"{what}: {self.batches} batches, {self.rows} rows, worst |1-cos| = {self.dcos:.3e}, worst abs diff = "
              f"{self.dabs:.3e}, {n_cu} CUs, {time.perf_counter() - self.t0:.2f} s")


def run_token_rows(e, m, batch, precision, what, tally=None):
    """Every token of the batch through encode_spans, held to check_rows (TOL and the bits of repeats). Returns the rows."""
    from encoder_rows_case import check_rows
    from voitta_rag_amd import encoder as enc

    t0 = time.perf_counter()
    seqs, which = batch
    distinct, row = token_index(seqs, which)
    got = enc.encode_spans(e, *token_spans(seqs))
    dcos, dabs = check_rows(got, m.token_rows(distinct), row, precision)
    if tally:
        tally.add(len(got), dcos, dabs)
    print(f"{m.name} {precision} {what}: {len(got)} rows, worst |1-cos| = {dcos:.3e}, worst abs diff = {dabs:.3e}, "
          f"{time.perf_counter() - t0:.2f} s")
    return got


def run_pooled(e, m, batch, pooling, precision, what, tally=None):
    from encoder_rows_case import check_rows
    from voitta_rag_amd import encoder as enc

    t0 = time.perf_counter()
    seqs, which = batch
    distinct, dense = distinct_of(seqs, which)
    got = enc.encode(e, *pack(seqs))
    dcos, dabs = check_rows(got, m.pooled_rows(distinct, pooling), dense, precision)
    if tally:
        tally.add(len(got), dcos, dabs)
    print(f"{m.name} {precision} {pooling} {what}: {len(got)} rows, worst |1-cos| = {dcos:.3e}, worst abs diff = {dabs:.3e}, "
          f"{time.perf_counter() - t0:.2f} s")
    return got


# ---- the catalogue of mistakes ---------------------------------------------------------------------------------------------
def _rotation(m, slip=False, next_frequency=False, no_minus=False, off=False, theta=None):
    """A "rotate" hook: rotate-half pairing with the layer's base, and one mistake."""
    def rotate(x, kind, layer):
        if off:
            return x
        S, dh = x.shape[1], x.shape[2]
        f = float(theta or m.theta(layer)) ** (-np.arange(0, dh, 2, dtype=np.float64) / dh)
        if next_frequency:
            f = np.roll(f, -1)
        pos = np.arange(S, dtype=np.float64)
        if slip and kind == "k":
            pos = np.where(pos >= 16, pos + 1, pos)
        cos, sin = np.cos(pos[:, None] * f[None, :]), np.sin(pos[:, None] * f[None, :])
        a, b = x[..., :dh // 2], x[..., dh // 2:]
        return np.concatenate([a * cos + b * sin if no_minus else a * cos - b * sin, b * cos + a * sin], axis=-1)

    return rotate


def _act(x, act):
    return x / (1.0 + np.exp(-x)) if act == "silu" else obert._gelu(x)


def _keys(m, layer):
    """Per family: the names of a layer's (norm gain ahead of or behind the attention block, norm gain of the FFN, FFN
    down projection)."""
    if m.family.startswith("nomic"):
        k = ro.layer_keys(layer)
        return k["ln1_g"], k["ln2_g"], k["down_w"]
    if m.family == "alibi":
        k = ao.layer_keys(layer)
        return k["ln1_g"], k["ln2_g"], k["f_w"]
    if m.family == "modernbert":
        k = mo.layer_keys(layer, LAYERS)
        return k.get("attn_norm"), k["mlp_norm"], k["wo_w"]
    k = t5.layer_keys(layer) if m.family == "t5" else qo.layer_keys(layer)
    return k["ln_a"], k["ln_m"], k["wo" if m.family == "t5" else "down"]


def _with(m, changed):
    w = dict(m.w64)
    w.update({k: np.ascontiguousarray(v, dtype=np.float64).view(_AsIs) for k, v in changed.items()})
    return w


def _gains_swapped(m):
    changed = {}
    for li in range(LAYERS):
        a, f, _ = _keys(m, li)
        if a is not None:
            changed[a], changed[f] = m.w64[f], m.w64[a]
    return dict(w=_with(m, changed))


def _folded_gain_of_the_wrong_layer(m):
    """The engine keeps the gain of the norm that layer li's Q/K/V projection folds in as layers[li - 1].ln2g. Read from
    layer li instead: a post-norm layer's closing LayerNorm takes the next layer's gain, a pre-norm layer's attention
    norm the next layer's (the last layer's: the final norm's)."""
    final = {"modernbert": "final_norm.weight", "t5": t5.FINAL_KEY, "qwen2": qo.FINAL_KEY}.get(m.family)
    changed = {}
    for li in range(1, LAYERS):
        if m.prenorm:
            changed[_keys(m, li)[0]] = m.w64[_keys(m, li + 1)[0] if li + 1 < LAYERS else final]
        else:
            changed[_keys(m, li - 1)[1]] = m.w64[_keys(m, li)[1]]
    return dict(w=_with(m, changed))


def _group_dropped(m):
    """Columns [I/2, I/2 + 16) of the middle layer's gated activation never reach the down projection."""
    name = _keys(m, 1)[2]
    down = np.array(m.w64[name], dtype=np.float64)
    down[:, m.I // 2:m.I // 2 + 16] = 0.0
    return dict(w=_with(m, {name: down}))


def _mean_subtracted(x, g, eps):
    c = x - x.mean(axis=-1, keepdims=True)
    return c / np.sqrt((c * c).mean(axis=-1, keepdims=True) + eps) * g


def _hook(name, make):
    return lambda m: dict(hooks={name: make(m)})


def _rotate_with(**how):
    return _hook("rotate", lambda m: _rotation(m, **how))


def _other(act):
    return "gelu" if act == "silu" else "silu"


_every = lambda m: True              # noqa: E731
_rotary = lambda m: m.rotary         # noqa: E731
_gated = lambda m: m.gated           # noqa: E731
_only = lambda family: (lambda m: m.family == family)  # noqa: E731

# name -> (applies(m), what(m) -> keyword arguments of Model.hidden)
MISTAKES = {
    "rotation: keys of rows >= 16 take the next row's position": (_rotary, _rotate_with(slip=True)),
    "rotation: pair j with pair j + 1's frequency": (_rotary, _rotate_with(next_frequency=True)),
    "rotation: rotate-half without the minus sign": (_rotary, _rotate_with(no_minus=True)),
    "rotation: none at all": (_rotary, _rotate_with(off=True)),
    "rotation: the local theta on a global layer": (_only("modernbert"),
                                                    _hook("rotate", lambda m: _rotation(m, theta=m.shape.theta_local))),
    "gate: gate and up halves swapped": (_gated, _hook("glu", lambda m: lambda g, u, li: _act(u, m.act) * g)),
    "gate: activation on the wrong half": (_gated, _hook("glu", lambda m: lambda g, u, li: g * _act(u, m.act))),
    "gate: one 16-column group dropped in the middle layer": (_gated, _group_dropped),
    "gate: SiLU and GELU exchanged": (_gated, _hook("glu", lambda m: lambda g, u, li: _act(g, _other(m.act)) * u)),
    "norm: the two gains of a layer swapped": (_every, _gains_swapped),
    "norm: the folded norm's gain from the wrong layer": (_every, _folded_gain_of_the_wrong_layer),
    "norm: RMSNorm with the mean subtracted": (lambda m: m.rms, _hook("rms", lambda m: _mean_subtracted)),
    "norm: the final norm skipped": (lambda m: m.prenorm, _hook("skip_final", lambda m: True)),
    "residual: the FFN's taken from before the attention block": (_every, _hook("stale_residual", lambda m: True)),
    "t5: GELU in place of ReLU": (_only("t5"), _hook("act", lambda m: lambda x, li: obert._gelu(x))),
    "qwen2: query head j reads KV head j % n_kv": (_only("qwen2"),
                                                   _hook("kv_of", lambda m: np.arange(m.shape.heads) % m.shape.kv_heads)),
}
