"""TEST INFRASTRUCTURE shared by test_attention_cpu.py and test_attention_gpu.py: models in which ONE attention layer
dominates every token row, the lengths that cross each attention kernel's edges, and a catalogue of the mistakes an
attention kernel makes.

A wrong key-validity mask, a window or causal edge off by one, a bias read one slot off or a dropped 16-key group moves
an ordinary model's token rows by less than test_encoder_gpu.TOL once a sequence is longer than about a hundred tokens:
one key of S weighs 1 / S in a context vector that is itself a small part of the row. Here the value and output
projections of one layer are scaled up, the feed-forward block's down projection is zero, the value and output biases
are zero, and so is what every token shares ahead of V (the embedding LayerNorm's shift, the token-type row): the context
is the weighted mean of value rows that share nothing, and all ids of a sequence are distinct (no two value rows
repeat), so that the row IS the context vector. Every projection matrix holds f16 values, so that f16 operands round
activations only. Every token is exposed as a one-token span of encode_spans.

The catalogue's functions return the additive [heads, S, S] array (the state's own bias or mask with one mistake built
in, in one head) that the oracles take as bias=; they are applied to the oracle only. test_attention_cpu.py proves, on
the CPU, that every mistake moves an exposed row of every query tile it touches by more than twice TOL while f16
operands leave the rows within half of TOL[f16]: the GPU suite would fail on a kernel that makes it.

Kernel states and their oracles: none — oracle.bert; window — modernbert_oracle (two layers, global_every = 2: layer 1
is the windowed one and the dominant one, layer 0 is kept quiet by a small W_o so that layer 1 still sees distinct
tokens); table — mpnet_oracle; slopes — alibi_oracle; causal — qwen2_oracle. Each at head size 64 (2 heads) and 32
(4 heads), H = 128, the narrowest model the engine loads. Head size 128 exists in the states none and causal alone
(launch_attention refuses it a window, a table and slopes): both are the Qwen3 body of qwen3_oracle with causal = 0 or 1,
H = 128 and two heads of 128 (an attention width of 256, not H), through the Q/K RMSNorm as real checkpoints run it."""
from __future__ import annotations

import dataclasses

import numpy as np

import alibi_oracle as ao
import modernbert_oracle as mo
import mpnet_oracle as mp
import qwen2_oracle as qo
import qwen3_oracle as q3
from oracle import bert as obert
from rope_oracle import f16_operand

H, I = 128, 128
STATES = ("none", "window", "table", "slopes", "causal")
HEAD_SIZES = (64, 32)  # the head sizes of all five states
WIDE, WIDE_STATES = 128, ("none", "causal")  # head size 128: the two states launch_attention has an instantiation for
PAIRS = [(state, dh) for state in STATES for dh in HEAD_SIZES] + [(state, WIDE) for state in WIDE_STATES]  # the models
VOCAB = 1408     # >= the longest sequence: all ids of a sequence are distinct
MAX_POS = 1408
NEG = -np.inf

# ---- lengths -------------------------------------------------------------------------------------------------------------
# Each number restates a constant of csrc/encoder.hip and has to follow it.
#   1 / 15 / 16 / 17        one 16-query tile (an MFMA tile; the CLS tail's q_limit = 16), one query more
#   63 / 64 / 65            one 64-key tile of all three kernels, one 64-query block of attention_kernel, one key more
#   127 / 128 / 129         two tiles; one 128-query block of attention_stream_kernel
ALL_KERNELS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129)
#   193                     attention_kernel: a fourth 64-query block that holds one query
F32_ONLY = (193,)
F32_LONGEST = 257  # the one longer length of the f32 and f16x3 ladders
#   79 / 80 / 81            attention_seq_kernel, NW = 4 waves: wave 0's second query tile (tile 4) with 15, 16, 17 queries
#   159 / 160 / 161         d_h = 64: one staging round holds 20 16-byte loads per thread = 160 keys (NST = 20 / NW)
#   320 / 321               d_h = 32: the same round holds 320 keys
#   256 / 257, 512 / 513    4 lds_keys d_h bytes cross the 64 KiB default (the hipFuncSetAttribute opt-in)
#   639 / 640, 1280         the last staged lengths: 4 * 640 * 64 = 4 * 1280 * 32 = 160 KiB of LDS
#   d_h = 128 (CH = 16 chunks per 256-byte row, its own swizzle: kswz = r & 15, vswz = (r & 7) << 1):
#   79 / 80 / 81            one staging round holds NST * NT / CH = 5 * 256 / 16 = 80 keys: 81 tokens (keys_pad = 96) take
#                           a second round; and wave 0's second query tile as above
#   160 / 161               keys_pad = 160 is two rounds, 176 a third
#   128 / 129               (of ALL_KERNELS) 4 lds_keys * 128 bytes: 65,536 at 128 keys, 73,728 at lds_keys = 144 — the opt-in
#   319 / 320               the last staged lengths: 4 * 320 * 128 = 160 KiB
STAGED = {64: (79, 80, 81, 159, 160, 161, 256, 257, 639, 640), 32: (79, 80, 81, 320, 321, 512, 513, 1280),
          128: (79, 80, 81, 160, 161, 319, 320)}
#   641 / 705 / 769         attention_stream_kernel at d_h = 64: the first streamed length (a sixth 128-query block and an
#                           eleventh key tile that hold one token), 705 = 11 * 64 + 1, 769 = 6 * 128 + 1 = 12 * 64 + 1
#   1281 / 1345             the same at d_h = 32 (1281 = 10 * 128 + 1 = 20 * 64 + 1, 1345 = 21 * 64 + 1)
#   321 / 337 / 385 / 449   the same at d_h = 128 (a ring of 4 * 64 * 128 halfs = 65,536 bytes of static LDS, NLD = 64 CH / NT
#                           = 4 loads per thread and tile): 321 = 2 * 128 + 65 = 5 * 64 + 1, a third block and a sixth key
#                           tile that hold one token past a full tile; 337 = 2 * 128 + 64 + 17: wave 2 of the third block
#                           (qw = 320), whose second query tile holds one query; 385 = 3 * 128 + 1 = 6 * 64 + 1;
#                           449 = 7 * 64 + 1
STREAMED = {64: (641, 705, 769), 32: (1281, 1345), 128: (321, 337, 385, 449)}
#   383 / 384 / 385 / 449   kWindowStreamFrom = 384: a windowed layer takes attention_stream_kernel from there on;
#                           449 = 7 * 64 + 1: with w = 8 the block's last query meets tiles in which it sees nothing
#                           (the softmax_base guard)
WINDOW_STREAM = (383, 384, 385, 449)
WINDOWS = (8, 64, 100)
#   R = 5 / 64 / 128 / 512  bias_tile's far-tile shortcut engages from `radius` keys on; kMaxBiasRadius = 512
#   640 at d_h = 64, R = 512: 4 * 640 * 64 + 4 * 1025 bytes exceed the LDS — the table tips the launch to the streamed kernel
RADII = (5, 64, 128, 512)
SLOPES = {64: (0.5, 0.1), 32: (0.5, 0.1, 0.25, 0.02)}
WIDE_GAIN = 0.5  # on the Q and K gains of the head-size-128 models (Model)
KERNEL_SPLIT = 262144  # kMaxChunkTokens: forward_all starts another chunk (seq0, tok_base > 0) beyond this many tokens


def ladder(dh, precision):
    """The lengths of one head size and precision, sorted."""
    if precision != "f16":
        return sorted(set(ALL_KERNELS + F32_ONLY + (F32_LONGEST,)))
    return sorted(set(ALL_KERNELS + F32_ONLY + STAGED[dh] + STREAMED[dh]))


def cases(state, dh, precision):
    return list(dict.fromkeys(_cases(state, dh, precision)))


def _cases(state, dh, precision):
    """(param, S) pairs of a model: param is the half-width w (window), the radius R (table), else None. One value of the
    parameter walks the whole ladder, the others the lengths at which they change what a kernel does."""
    full = ladder(dh, precision)
    top = full[-1]
    if state == "window":
        some = [s for s in (17, 65, 129) + WINDOW_STREAM if s <= top]
        return ([(64, s) for s in sorted(set(full + [s for s in WINDOW_STREAM if s <= top]))] + [(8, s) for s in some]
                + [(100, s) for s in some if s > 100])
    if state == "table":
        longest = [s for s in ((640, 705) if dh == 64 else (1280, 1345)) if s <= top] or [top]
        return ([(64, s) for s in full] + [(5, s) for s in (17, 65, 129)] + [(128, s) for s in (129, 193, 257)]
                + [(128, s) for s in longest[-1:]] + [(512, s) for s in longest])
    return [(None, s) for s in full]


def sequence(S):
    """S distinct ids, the same for every model."""
    return np.random.default_rng(1000 + S).permutation(VOCAB)[:S].astype(np.int32)


# ---- the state's own bias or mask ----------------------------------------------------------------------------------------
def _dist(S, cols=None):
    pos = np.arange(S)
    return np.arange(cols or S)[None, :] - pos[:, None]  # key - query


def window_mask(heads, S, w, cols=None):
    return np.broadcast_to(np.where(np.abs(_dist(S, cols)) <= w, 0.0, NEG), (heads, S, cols or S)).copy()


def causal_mask(heads, S, cols=None):
    return np.broadcast_to(np.where(_dist(S, cols) <= 0, 0.0, NEG), (heads, S, cols or S)).copy()


def table_bias(table, S, cols=None, shift=0, clamp=None, mirrored=False):
    table = np.asarray(table, np.float64)
    R = (table.shape[1] - 1) // 2
    c = R if clamp is None else clamp
    d = -_dist(S, cols) if mirrored else _dist(S, cols)
    return table[:, np.clip(np.clip(d, -c, c) + R + shift, 0, 2 * R)]


def slope_bias(slopes, S, cols=None):
    return -np.asarray(slopes, np.float64)[:, None, None] * np.abs(_dist(S, cols))[None].astype(np.float64)


# ---- the models ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Model:
    state: str
    dh: int
    v_scale: float = 32.0
    o_scale: float = 32.0

    def __post_init__(self):
        self.heads = 2 if self.dh == WIDE else H // self.dh
        seed = 7000 + 10 * STATES.index(self.state) + self.dh + RESEED.get((self.state, self.dh), 0)
        s = self.state
        if self.dh == WIDE:
            # the Qwen3 body, causal or not: hidden 128, two heads of 128 (A = 256, not H) each with K/V rows of its own
            # (the two heads' value rows share nothing, FAULT_HEAD exists), Q/K RMSNorm on. Made to dominate as the
            # causal model below; no q/k/v biases exist
            assert s in WIDE_STATES, (s, self.dh)
            self.shape = q3.Qwen3Shape(1, H, self.heads, self.heads, I, WIDE, qk_norm=True, vocab=VOCAB)
            w = q3.random_weights(self.shape, seed)
            k = q3.layer_keys(0)
            # (behind the norm the gains alone size the logits, about g_q g_k sqrt(d_h) cos(q, k) with cos of order
            # d_h^-1/2: qwen3_oracle's gains around 0.9 give logits of order one; WIDE_GAIN times them a quarter of that,
            # oracle.bert's seeded scale as for the causal model below — a key's weight within a small factor of 1 / S)
            for name in ("qn", "kn"):
                w[k[name]] = w[k[name]] * np.float32(WIDE_GAIN)
            w[k["v"]] = w[k["v"]] * np.float32(self.v_scale)
            w[k["o"]] = w[k["o"]] * np.float32(self.o_scale)
            w[k["down"]] = np.zeros_like(w[k["down"]])
        elif s == "none":
            self.shape = obert.BertShape(1, H, self.heads, I, vocab=VOCAB, max_pos=MAX_POS)
            w = obert.random_weights(self.shape, seed)
            k = obert.layer_keys(0)
            self._dominate(w, k["v_w"], k["v_b"], k["o_w"], k["o_b"], k["f_w"], k["f_b"], obert.EMB_KEYS["ln_b"],
                           obert.EMB_KEYS["type"])
        elif s == "table":
            self.shape = mp.MpnetShape(1, H, self.heads, I, vocab=VOCAB, positions=MAX_POS + mp.POS_START)
            w = mp.random_weights(self.shape, seed)
            k = mp.layer_keys(0)
            self._dominate(w, k["v_w"], k["v_b"], k["o_w"], k["o_b"], k["f_w"], k["f_b"], mp.EMB_KEYS["ln_b"])
            rng = np.random.default_rng(seed + 1)
            self.tables = {R: rng.normal(0, 1.0, (self.heads, 2 * R + 1)).astype(np.float32) for R in RADII}
        elif s == "slopes":
            self.shape = ao.AlibiShape(1, H, self.heads, I, vocab=VOCAB, max_pos=MAX_POS)
            w = ao.random_weights(self.shape, seed)
            k = ao.layer_keys(0, self.shape.ffn)
            self._dominate(w, k["v_w"], k["v_b"], k["o_w"], k["o_b"], k["f_w"], k["f_b"], ao.EMB_KEYS["ln_b"],
                           ao.EMB_KEYS["type"])
            self.slopes = np.asarray(SLOPES[self.dh], np.float32)
        elif s == "window":
            self.shape = mo.ModernShape(2, H, self.heads, I, vocab=VOCAB, max_pos=MAX_POS, window=64, global_every=2)
            w = mo.random_weights(self.shape, seed)
            k0, k1 = mo.layer_keys(0, 2), mo.layer_keys(1, 2)
            w[k0["o_w"]] = w[k0["o_w"]] * np.float32(0.25)  # layer 0 quiet: layer 1 still sees distinct tokens
            w[k0["wo_w"]] = np.zeros_like(w[k0["wo_w"]])
            rows = w[k1["qkv_w"]].copy()
            rows[2 * H:] *= np.float32(self.v_scale)
            w[k1["qkv_w"]] = rows
            w[k1["o_w"]] = w[k1["o_w"]] * np.float32(self.o_scale)
            w[k1["wo_w"]] = np.zeros_like(w[k1["wo_w"]])
        else:
            self.shape = qo.Qwen2Shape(1, H, self.heads, self.heads, I, vocab=VOCAB)
            w = qo.random_weights(self.shape, seed)
            k = qo.layer_keys(0)
            # (qwen2_oracle draws logits of order one; a quarter of that is oracle.bert's seeded scale: a key's weight
            # then stays within a small factor of 1 / S, so that no single key of a long sequence is negligible)
            for name in ("q", "qb", "k", "kb"):
                w[k[name]] = w[k[name]] * np.float32(0.5)
            w[k["v"]] = w[k["v"]] * np.float32(self.v_scale)
            w[k["vb"]] = np.zeros_like(w[k["vb"]])
            w[k["o"]] = w[k["o"]] * np.float32(self.o_scale)
            w[k["down"]] = np.zeros_like(w[k["down"]])
        # every projection matrix holds f16 values: an f16-operand product reads them as they are, which takes the
        # weights' rounding out of the f16 noise that condition (b) of test_attention_cpu.py bounds
        self.w = {k: v.astype(np.float16).astype(np.float32) if v.ndim == 2 and "layer" in k else v for k, v in w.items()}
        self._rows = {}

    def _dominate(self, w, v_w, v_b, o_w, o_b, *zero):
        """V and W_o scaled up; zero: the value and output biases, the FFN's down projection, and what all tokens of a
        sequence share ahead of V (the embedding LayerNorm's shift, the token-type row): a shared part of the value rows
        does not shrink with the sequence's length as their mean does, and would hide one key of a long sequence."""
        w[v_w] = w[v_w] * np.float32(self.v_scale)
        w[o_w] = w[o_w] * np.float32(self.o_scale)
        for name in (v_b, o_b) + zero:
            w[name] = np.zeros_like(w[name])

    @property
    def name(self):
        return f"{self.state}-d{self.dh}"

    # -- the oracle --
    def own_bias(self, S, param, cols=None):
        """The state's own additive array [heads, S, cols or S] (zeros for `none`)."""
        if self.state == "window":
            return window_mask(self.heads, S, param, cols) if param else np.zeros((self.heads, S, cols or S))
        if self.state == "causal":
            return causal_mask(self.heads, S, cols)
        if self.state == "table":
            return table_bias(self.tables[param], S, cols) if param else np.zeros((self.heads, S, cols or S))
        if self.state == "slopes":
            return slope_bias(self.slopes, S, cols) if param != "off" else np.zeros((self.heads, S, cols or S))
        return np.zeros((self.heads, S, cols or S))

    def hidden(self, seq, param=None, bias=None, operand=None):
        """The oracle's final hidden states [S, H], f64. bias: the complete additive array in place of the state's own
        (a catalogue mistake); operand: rope_oracle.f16_operand for the f16-operand run, P included."""
        S = len(seq)
        if bias is None:
            bias = self.own_bias(S, param)
        s = self.state
        if self.dh == WIDE:  # (the mask is the bias's alone, as for the causal model)
            return q3.encode_one(self.w, self.shape, seq, causal=False, bias=bias, operand=operand)
        if s == "none":
            return obert.encode_one(self.w, self.shape, seq, bias=bias, operand=operand)
        if s == "table":
            return mp.encode_one(self.w, self.shape, seq, table=None, bias=bias, operand=operand)
        if s == "slopes":
            return ao.encode_one(self.w, self.shape, seq, None, bias=bias, operand=operand)
        if s == "causal":
            return qo.encode_one(self.w, self.shape, seq, causal=False, bias=bias, operand=operand)
        # window: layer 1 stays a windowed layer (its rotary base) with the oracle's own mask wider than any sequence:
        # the mask is the bias's alone, mistakes included. No window (0): the global model.
        shape = dataclasses.replace(self.shape, window=MAX_POS if param else 0)
        return mo.encode_one(self.w, shape, seq, operand=operand, bias=bias, bias_layer=1, round_p=True)

    def rows(self, S, param=None):
        """Unit-length oracle rows of sequence(S), memoised and read-only."""
        key = (S, param)
        if key not in self._rows:
            r = unit(self.hidden(sequence(S), param))
            r.setflags(write=False)
            self._rows[key] = r
        return self._rows[key]

    # -- the engine --
    def desc(self, precision, pooling="mean", param=None, **over):
        s = self.state
        if self.dh == WIDE:
            return q3.desc_for(self.shape, pooling, precision, max_pos=MAX_POS, causal=int(s == "causal"), **over)
        if s == "none":
            sh = self.shape
            from voitta_rag_amd import encoder as enc

            return enc.BertDesc(sh.layers, sh.hidden, sh.heads, sh.intermediate, vocab=sh.vocab, max_pos=sh.max_pos,
                                type_vocab=sh.type_vocab, pooling=pooling, normalize=True, eps=sh.eps, precision=precision,
                                **over)
        if s == "table":
            return mp.desc_for(self.shape, pooling, precision, **over)
        if s == "slopes":
            return ao.desc_for(self.shape, pooling, precision, max_pos=MAX_POS, attention_slopes=self.slopes, **over)
        if s == "window":
            return mo.desc_for(dataclasses.replace(self.shape, window=param or 0), pooling, precision, **over)
        return qo.desc_for(self.shape, pooling, precision, max_pos=MAX_POS, **over)

    def engine(self, precision, pooling="mean", param=None, **over):
        """An engine with the model loaded through load_encoder. param: the window's half-width (part of the
        description); a table is set afterwards (set_param)."""
        from voitta_rag_amd import Engine
        from voitta_rag_amd import encoder as enc

        e = Engine(H)
        desc = self.desc(precision, pooling, param, **over)
        state = enc.mpnet_slots(self.w, desc)[0] if self.state == "table" else self.w
        enc.load_encoder(e, desc, state)
        return e

    def set_param(self, e, param):
        """The table of radius `param` on engine e (None: no table); the slopes on ("on") or off ("off")."""
        if self.state == "table":
            e.set_attention_bias(self.tables[param] if param else None)
        elif self.state == "slopes":
            e.set_attention_slopes(None if param == "off" else self.slopes)


# seeds moved on where the first draw left the f16 noise of one length above TOL / 2 (condition (b))
RESEED = {("none", 32): 3000, ("causal", 64): 1000}
_MODELS = {}


def model(state, dh):
    if (state, dh) not in _MODELS:
        _MODELS[state, dh] = Model(state, dh)
    return _MODELS[state, dh]


def unit(rows):
    return rows / np.linalg.norm(rows, axis=-1, keepdims=True)


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.int32), off


def token_rows(e, seqs):
    """Every token of every sequence as a one-token span of encode_spans: [sum of lengths, H]."""
    from voitta_rag_amd import encoder as enc

    ids, off = pack(seqs)
    tok = np.concatenate([np.stack([np.arange(len(s)), np.arange(len(s)) + 1], axis=1) for s in seqs]).astype(np.int32)
    return enc.encode_spans(e, ids, off, off, tok)


def deviation(got, want):
    """(|1 - cos|, largest absolute difference) per row."""
    got = np.asarray(got, np.float64)
    cos = (got * want).sum(-1) / np.linalg.norm(got, axis=-1) / np.linalg.norm(want, axis=-1)
    return np.abs(1.0 - cos), np.abs(got - want).max(axis=-1)


# ---- the fault catalogue -------------------------------------------------------------------------------------------------
# Every function takes (model, S, param) and returns the complete additive array with the mistake in head FAULT_HEAD, or
# None where the mistake changes nothing at this length (or would leave a query without a key).
FAULT_HEAD = 1
MATERIAL = 3.0


def _own(m, S, param):
    return m.own_bias(S, param)


def last_key_invisible(m, S, param):
    b = _own(m, S, param)
    b[FAULT_HEAD, :, S - 1] = NEG
    return b


PHANTOM_MIN = 15


def phantom_key(m, S, param):
    """Zero keys and values behind the end, up to the end of the 64-key tile, as a failed `key < len` test admits them
    (the f32 and the streamed kernel stage a tile's missing rows as zeros): as many columns more, with the state's own
    bias for those offsets in the faulty head and -inf in the others. Zero keys only SCALE a head's context, by
    1 - n / S for n of them at equal weights, and a row that is the normalised context shows a scaling through the
    balance of the heads alone: one zero key of 640 moves a row by 0.3 x TOL, below what f16 noise allows any test to
    see. So the mistake is planted where it admits at least PHANTOM_MIN keys (lengths up to 49 past a tile's start), and
    faults() judges it in the last query tile, which sees most of them under a window or slopes."""
    n = -S % 64
    if n < PHANTOM_MIN:
        return None
    b = m.own_bias(S, param, cols=S + n)
    for h in range(m.heads):
        if h != FAULT_HEAD:
            b[h, :, S:] = NEG
    return b


def _last_tiles(S):
    return (S - 1) // 16, (S - 1) // 64


def first_key_of_tile_dropped(m, S, param):
    qt, kt = _last_tiles(S)
    b = _own(m, S, param)
    b[FAULT_HEAD, 16 * qt:16 * qt + 16, 64 * kt] = NEG
    return b


def last_group_dropped(m, S, param):
    qt, _ = _last_tiles(S)
    g = (S - 1) // 16  # the last 16-key group the sequence's last tile holds
    b = _own(m, S, param)
    b[FAULT_HEAD, 16 * qt:16 * qt + 16, 16 * g:16 * g + 16] = NEG
    return b


def first_tile_last_group_dropped(m, S, param):
    """Keys 48 .. 63 of the first tile, for the first query tile behind them (causal: one that sees them)."""
    if S <= 64:
        return None
    b = _own(m, S, param)
    b[FAULT_HEAD, 64:80, 48:64] = NEG
    return b


def neighbour_rows(m, S, param):
    """The last-but-one query tile takes the bias or mask rows of the tile behind it (none: nothing to take)."""
    qt = (S - 1) // 16 - 1
    if qt < 0 or m.state == "none":
        return None
    full = m.own_bias(S + 16, param)[:, :, :S]
    b = _own(m, S, param)
    b[FAULT_HEAD, 16 * qt:16 * qt + 16] = full[FAULT_HEAD, 16 * qt + 16:16 * qt + 32]
    return b


def window_too_wide(m, S, param):
    b = _own(m, S, param)
    d = _dist(S)
    b[FAULT_HEAD][d == param + 1] = 0.0  # the far side only
    return b


def window_too_narrow(m, S, param):
    b = _own(m, S, param)
    b[FAULT_HEAD][_dist(S) == -param] = NEG  # the near side only
    return b


def causal_one_ahead(m, S, param):
    b = _own(m, S, param)
    b[FAULT_HEAD][_dist(S) == 1] = 0.0  # j <= i + 1
    return b


def causal_strict(m, S, param):
    b = _own(m, S, param)
    d = _dist(S)
    b[FAULT_HEAD][(d == 0) & (np.arange(S)[:, None] > 0)] = NEG  # j < i (query 0 keeps its only key)
    return b


def causal_diagonal_group_dropped(m, S, param):
    """The 16-key group that holds a query tile's own diagonal, keys 16 qt .. 16 qt + 15, dropped for that tile: a causal
    key loop that ends one group early (kt1 or nt of attention_seq_kernel, `kt <= qw + 31` of attention_stream_kernel).
    Planted in the last-but-one query tile and in tile 4 (queries 64 .. 79: wave 0's second tile in the staged kernel,
    wave 2's first in the streamed one) where the sequence reaches it; only in tiles qt >= 1, whose queries keep the
    keys below 16 qt."""
    tiles = {qt for qt in ((S - 1) // 16 - 1, 4) if qt >= 1 and 16 * qt < S}
    if not tiles:
        return None
    b = _own(m, S, param)
    for qt in tiles:
        b[FAULT_HEAD, 16 * qt:16 * qt + 16, 16 * qt:16 * qt + 16] = NEG
    return b


def _table_fault(m, S, param, **how):
    b = _own(m, S, param)
    b[FAULT_HEAD] = table_bias(m.tables[param], S, **how)[FAULT_HEAD]
    return b


def table_mirrored(m, S, param):
    return _table_fault(m, S, param, mirrored=True)


def table_clamp_short(m, S, param):
    return _table_fault(m, S, param, clamp=param - 1)


def table_shifted(m, S, param):
    return _table_fault(m, S, param, shift=1)


def table_far_tile_early(m, S, param):
    """bias_tile's shortcut (one far value for a whole 64-key tile of a 16-query tile) engaging 16 keys early."""
    b = _own(m, S, param)
    t = m.tables[param].astype(np.float64)[FAULT_HEAD]
    R = param
    for q0 in range(0, S, 16):
        for k0 in range(0, S, 64):
            if k0 - (q0 + 15) >= R - 16:
                b[FAULT_HEAD, q0:q0 + 16, k0:k0 + 64] = t[2 * R]
            elif q0 - (k0 + 63) >= R - 16:
                b[FAULT_HEAD, q0:q0 + 16, k0:k0 + 64] = t[0]
    return b


def slope_distance_off_by_one(m, S, param):
    b = _own(m, S, param)
    b[FAULT_HEAD] = -float(m.slopes[FAULT_HEAD]) * np.abs(_dist(S) + 1)
    return b


def slope_group_start(m, S, param):
    """The distance taken from the lane's group start (key & ~3, `r` dropped) for the last query tile."""
    qt, _ = _last_tiles(S)
    b = _own(m, S, param)
    pos = np.arange(S)
    d = (pos & ~3)[None, :] - pos[:, None]
    b[FAULT_HEAD, 16 * qt:16 * qt + 16] = (-float(m.slopes[FAULT_HEAD]) * np.abs(d))[16 * qt:16 * qt + 16]
    return b


GEOMETRY_FAULTS = (last_key_invisible, phantom_key, first_key_of_tile_dropped, last_group_dropped,
                   first_tile_last_group_dropped, neighbour_rows)
STATE_FAULTS = {"none": (), "window": (window_too_wide, window_too_narrow),
                "causal": (causal_one_ahead, causal_strict, causal_diagonal_group_dropped),
                "table": (table_mirrored, table_clamp_short, table_shifted, table_far_tile_early),
                "slopes": (slope_distance_off_by_one, slope_group_start)}


def faults(m, S, param):
    """(name, additive array, touched 16-query tiles) of every catalogue mistake that applies to (model, S, param): one
    that changes a logit some query sees and leaves every query a key."""
    own = m.own_bias(S, param)
    out = []
    for f in GEOMETRY_FAULTS + STATE_FAULTS[m.state]:
        b = f(m, S, param)
        if b is None:
            continue
        if not np.isfinite(b).any(axis=-1).all():
            continue  # a query of the faulty head would see no key at all
        # a changed logit counts where it can matter: the key's bias, right or wrong, within MATERIAL of the largest bias
        # of its row (a key 100 positions away under a slope of 0.5 weighs exp(-50): no kernel's mistake there can show),
        # and not where the row's visible keys all change by the same amount (a softmax does not move: one key alone)
        square = b[:, :, :S]
        floor = own.max(axis=-1, keepdims=True) - MATERIAL
        same = (square == own) | (np.isinf(square) & np.isinf(own))
        with np.errstate(all="ignore"):
            delta = np.where(np.isfinite(square) & np.isfinite(own), square - own, np.nan)
            spread = np.nanmax(delta, axis=-1, initial=-np.inf) - np.nanmin(delta, axis=-1, initial=np.inf)
        uniform = (np.isfinite(square) == np.isfinite(own)).all(axis=-1) & ~(spread > 1e-12)
        differs = ~same & (np.maximum(square, own) >= floor) & ~uniform[..., None]
        changed = differs.any(axis=(0, 2))
        if b.shape[-1] > S:
            changed[:] = False
            changed[16 * ((S - 1) // 16):] = (b[:, 16 * ((S - 1) // 16):, S:] >= floor[:, 16 * ((S - 1) // 16):]).any(axis=(0, 2))
        if not changed.any():
            continue
        out.append((f.__name__, b, sorted(set((np.flatnonzero(changed) // 16).tolist()))))
    return out


def f16_rows(m, S, param=None):
    """The oracle's rows with every matrix product reading f16 operands, the probabilities included."""
    return unit(m.hidden(sequence(S), param, operand=f16_operand))
