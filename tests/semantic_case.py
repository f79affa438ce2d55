"""What the semantic chunking tests share (test_semantic_cpu.py asserts the fixtures' margins, test_semantic_gpu.py runs
them): tiny seeded models with their f64 hidden states, planted documents whose topic switches the oracle sees with room
to spare, and the bound a device distance is held to.

A planted document: units of 4..11 tokens, every token of a unit the same vocabulary entry (its topic's), the topic
changing behind `switches` of the units. With buffer 0 a switch gap is several times as far as any other gap."""
import functools

import numpy as np

import qwen2_oracle as qo
import rope_oracle as ro
import semantic_oracle as so
from oracle import bert as obert
from test_encoder_gpu import TOL  # (cosine, per component) per precision: the project's bar for an embedding row


def distance_bound(hidden_size: int, precision: str) -> float:
    """2 sqrt(H) TOL: the device's normalised combined vectors lie within TOL (per component) of the oracle's, so each
    within sqrt(H) TOL in length, and the dot of two unit vectors moves by at most the sum of the two."""
    return 2.0 * np.sqrt(hidden_size) * TOL[precision][1]


class Model:
    """kind: bert128 / bert384 / bert1024 (post-norm BERT, H as named), bertlong (bert128 with 2112 positions, 1 layer),
    bertzero (bert128 whose last LayerNorm has zero weight and bias: every hidden row is zero), rope64 (rotary, for the
    streamed-attention route), qwen2 (a causal body)."""

    def __init__(self, kind):
        self.kind = kind
        self.oracle = obert
        if kind in ("bert128", "bertzero"):
            self.shape = obert.BertShape(2, 128, 2, 256, vocab=64, max_pos=512)
        elif kind == "bertlong":
            self.shape = obert.BertShape(1, 128, 2, 256, vocab=64, max_pos=2112)
        elif kind == "bert384":
            self.shape = obert.BertShape(2, 384, 6, 256, vocab=64, max_pos=512)
        elif kind == "bert1024":
            self.shape = obert.BertShape(1, 1024, 16, 128, vocab=64, max_pos=512)
        elif kind == "rope64":
            self.shape, self.oracle = ro.RopeShape(2, 128, 2, 256, vocab=64, max_pos=2048), ro
        elif kind == "qwen2":
            self.shape, self.oracle = qo.Qwen2Shape(2, 128, 2, 2, 256, vocab=64), qo
        else:
            raise KeyError(kind)
        self.w = self.oracle.random_weights(self.shape, 31)
        if kind == "bertzero":
            k = obert.layer_keys(self.shape.layers - 1)
            self.w[k["ln2_g"]] = np.zeros_like(self.w[k["ln2_g"]])
            self.w[k["ln2_b"]] = np.zeros_like(self.w[k["ln2_b"]])
        self.memo = {}

    @property
    def hidden_size(self):
        return self.shape.hidden

    def desc(self, precision, pooling="mean", **kw):
        from voitta_rag_amd import encoder as enc

        s = self.shape
        if self.oracle is obert:
            return enc.BertDesc(s.layers, s.hidden, s.heads, s.intermediate, vocab=s.vocab, max_pos=s.max_pos,
                                pooling=pooling, normalize=True, eps=s.eps, precision=precision, **kw)
        if self.oracle is ro:
            return ro.desc_for(s, pooling, precision)
        return qo.desc_for(s, pooling, precision)

    def hidden(self, seq):
        """last_hidden_state of one sequence in f64, computed once."""
        key = np.asarray(seq, np.int32).tobytes()
        if key not in self.memo:
            self.memo[key] = self.oracle.encode_one(self.w, self.shape, seq)
            self.memo[key].setflags(write=False)
        return self.memo[key]

    def engine(self, precision, pooling="mean", **kw):
        from voitta_rag_amd import Engine
        from voitta_rag_amd import encoder as enc

        e = Engine(self.shape.hidden)
        enc.load_encoder(e, self.desc(precision, pooling, **kw), self.w)
        return e


@functools.lru_cache(maxsize=None)
def model(kind) -> Model:
    return Model(kind)


def planted(n_units, switches, seed, lo=4, hi=12, lead=1, gap_every=0):
    """(ids, units, the set of units a topic switch precedes). lead: unowned tokens in front ([CLS]); one unowned token
    behind; gap_every > 0: an unowned token in front of every gap_every-th unit as well."""
    rng = np.random.default_rng(seed)
    sw = set(rng.choice(np.arange(1, n_units), size=switches, replace=False).tolist()) if switches else set()
    topic = int(rng.integers(0, 30))
    ids, units = [1] * lead, []
    for r in range(n_units):
        if r in sw:
            topic = (topic + int(rng.integers(1, 29))) % 30
        if gap_every and r % gap_every == gap_every - 1:
            ids.append(2)
        n = int(rng.integers(lo, hi))
        units.append((len(ids), len(ids) + n))
        ids += [2 * topic + 3] * n
    ids.append(2)
    return np.asarray(ids, np.int32), units, sw


def pack(seqs, units):
    """(ids, offsets, unit_off, unit_tok) of sequences and their unit lists."""
    ids = np.concatenate(seqs).astype(np.int32)
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    unit_off = np.zeros(len(seqs) + 1, np.int32)
    unit_off[1:] = np.cumsum([len(u) for u in units])
    flat = [be for own in units for be in own]
    return ids, off, unit_off, np.asarray(flat, np.int32).reshape(len(flat), 2)


class Fixture:
    """Sequences with units, the rule's parameters, and the precisions at which the oracle's decisions are held against
    the device's (the margins are then more than twice distance_bound; test_semantic_cpu asserts it)."""

    def __init__(self, name, kind, docs, params, precisions):
        self.name, self.kind, self.params, self.precisions = name, kind, params, precisions
        self.seqs = [d[0] for d in docs]
        self.units = [d[1] for d in docs]

    @property
    def model(self):
        return model(self.kind)

    def oracle(self):
        """per sequence (d, unit_start, un-normalised chunk means), f64"""
        return _oracle(self)

    def arrays(self):
        return pack(self.seqs, self.units)


@functools.lru_cache(maxsize=None)
def _oracle(fx):
    return [so.sequence(fx.model.hidden(s), u, fx.params) for s, u in zip(fx.seqs, fx.units)]


ALL = ("f32", "f16x3", "f16")
# 20 gaps at 200 permille: B = 4 = the switches; -floor: every gap inside the budget, min_distance deciding
FIXTURES = [
    Fixture("bert128-b0", "bert128", [planted(21, 4, s) for s in (0, 1, 2)], so.Params(0, 200), ALL),
    Fixture("bert128-b0-gaps", "bert128", [planted(21, 4, 3, gap_every=4), planted(11, 2, 4, lead=3)], so.Params(0, 200), ALL),
    Fixture("bert128-b0-floor", "bert128", [planted(21, 4, s) for s in (0, 2)], so.Params(0, 1000, min_distance=0.2), ALL),
    Fixture("bert128-b0-tokens", "bert128", [planted(21, 4, s) for s in (1, 2)],
            so.Params(0, 200, min_tokens=30, max_tokens=60), ALL),
    Fixture("bert384-b0", "bert384", [planted(21, 4, s) for s in (0, 1)], so.Params(0, 200), ALL),
    Fixture("bert1024-b0", "bert1024", [planted(21, 4, s) for s in (1, 2)], so.Params(0, 200), ALL),
    Fixture("qwen2-b0", "qwen2", [planted(21, 4, s) for s in (0, 1)], so.Params(0, 200), ALL),
    Fixture("bert128-b1", "bert128", [planted(21, 4, 2)], so.Params(1, 200), ("f32", "f16x3")),
]
BY_NAME = {f.name: f for f in FIXTURES}
