"""TEST INFRASTRUCTURE shared by test_cls_collapse_cpu.py and test_cls_collapse_gpu.py: the last layer of a
[CLS]-pooled model attended from the [CLS] row alone, on the hidden rows themselves (csrc/encoder.hip, `collapse` in
forward_chunk: cls_head_gemm_kernel, cls_attend_kernel).

collapsed_cls() restates that arithmetic in f64, with a hooks= keyword for planted mistakes, and with operand=
rope_oracle.f16_operand it rounds what the kernels round (the pre-LayerNorm rows, the weights, the [CLS] query, u, the
softmax weights times 1/sigma, z, the context). The model has two layers in the manner of attention_case.Model's window
state: layer 0 is kept quiet (a small W_o), layer 1 dominates the [CLS] row (V and W_o times 32, FFN-down zero, V and O
biases zero), all ids of a sequence are distinct and every projection matrix is on the f16 grid. Layer 0's FFN-down
matrix is planted: 1 a^T + v b^T, so that the pre-LayerNorm rows the last layer reads carry a mean and a sigma that
differ from token to token (an ordinary random model's rows all have nearly the same mean and sigma, and a mistake in
the mean or 1/sigma terms would then cancel in the softmax)."""
from __future__ import annotations

import math

import numpy as np

from oracle import bert as obert
from rope_oracle import f16_operand

H, I = 128, 128
HEAD_SIZES = (64, 32)
MAX_POS = 257
VOCAB = 1024

# ---- lengths: each number restates a constant of csrc/encoder.hip and has to follow it -------------------------------
#   kClsGroup = 16          keys per logit MFMA of cls_attend_kernel (15 / 16 / 17)
#   kClsStep = 32           keys per context MFMA, the padding of the staged key count (31 / 32 / 33)
#   64                      4 waves x kClsGroup: one round of pass 1; the lanes of the softmax's wave (63 / 64 / 65)
#   128 / MAX_POS           two and more rounds; 257 = 8 * 32 + 1: a ninth step that holds one key
CLS_GROUP, CLS_STEP, CLS_ROUND = 16, 32, 64
LADDER = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, MAX_POS)
KERNEL_SPLIT = 262144  # kMaxChunkTokens
CLS_HEADS = 16         # kClsHeads: more heads keep the ordinary route


def sequence(S, salt=0):
    """S distinct ids."""
    return np.random.default_rng(5000 + 7 * S + salt).permutation(VOCAB)[:S].astype(np.int32)


def ladder_batch():
    """Every ladder length twice, the second time behind an odd shift: other offsets inside the 128- and 256-row tiles."""
    lens = list(LADDER) + [3] + list(LADDER[::-1])
    return [sequence(S, i) for i, S in enumerate(lens)]


def pack(seqs):
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs).astype(np.int32), off


def unit(rows):
    return rows / np.linalg.norm(rows, axis=-1, keepdims=True)


def deviation(got, want):
    got = np.asarray(got, np.float64)
    cos = (got * want).sum(-1) / np.linalg.norm(got, axis=-1) / np.linalg.norm(want, axis=-1)
    return np.abs(1.0 - cos), np.abs(got - want).max(axis=-1)


# ---- the arithmetic ----------------------------------------------------------------------------------------------------
def _stats(x, eps):
    mu = x.mean(axis=-1)
    var = ((x - mu[..., None]) ** 2).mean(axis=-1)
    return mu, 1.0 / np.sqrt(var + eps)


def pre_rows(w, shape, ids, operand=None):
    """The pre-LayerNorm rows [S, H] in front of the LAST layer (the rows its closing LayerNorm of the layer before
    reads), computed as oracle.bert.encode_one computes them."""
    r = operand or (lambda a: a)
    W = lambda k: r(w[k].astype(np.float64)) if w[k].ndim == 2 and k.startswith("encoder.") else w[k].astype(np.float64)  # noqa: E731
    ids = np.asarray(ids, np.int64)
    S, nh = len(ids), shape.heads
    dh = shape.hidden // nh
    x = W(obert.EMB_KEYS["word"])[ids] + W(obert.EMB_KEYS["pos"])[:S] + W(obert.EMB_KEYS["type"])[0]
    x = obert._ln(x, W(obert.EMB_KEYS["ln_g"]), W(obert.EMB_KEYS["ln_b"]), shape.eps)
    pre, prev = None, None
    for i in range(shape.layers - 1):
        k = obert.layer_keys(i)
        if prev is not None:
            x = obert._ln(pre, W(prev["ln2_g"]), W(prev["ln2_b"]), shape.eps)
        xa = r(x)
        q = r((xa @ W(k["q_w"]).T + W(k["q_b"])).reshape(S, nh, dh).transpose(1, 0, 2))
        kk = r((xa @ W(k["k_w"]).T + W(k["k_b"])).reshape(S, nh, dh).transpose(1, 0, 2))
        v = r((xa @ W(k["v_w"]).T + W(k["v_b"])).reshape(S, nh, dh).transpose(1, 0, 2))
        s = q @ kk.transpose(0, 2, 1) / math.sqrt(dh)
        ctx = r(obert.attend(s, v, None, operand).transpose(1, 0, 2).reshape(S, shape.hidden))
        x = obert._ln(ctx @ W(k["o_w"]).T + W(k["o_b"]) + x, W(k["ln1_g"]), W(k["ln1_b"]), shape.eps)
        h = r(obert._gelu(r(x) @ W(k["i_w"]).T + W(k["i_b"])))
        pre = h @ W(k["f_w"]).T + W(k["f_b"]) + x
        prev = k
    return pre


def collapsed_cls(w, shape, ids, operand=None, hooks=None, phantom=None):
    """The final hidden row of the [CLS] token, [H] f64, by steps 1-4 of the collapsed last layer.
    hooks: a dict of planted mistakes —
      "keys": f(S) -> bool [S], the keys admitted          "no_mean_alpha": the mean_j alpha_h term missing
      "no_cs_gamma": the cs_v gamma_h term missing          "inv_shift" / "mean_shift": d, statistics of row j + d
      "u_head_shift": u of head h used for head h + 1       "no_inv_in_w": 1/sigma_j missing from the weights w_hj
    phantom: the pre-LayerNorm rows of another sequence whose first row joins the keys."""
    hooks = hooks or {}
    r = operand or (lambda a: a)
    f = lambda k: w[k].astype(np.float64)  # noqa: E731
    L, Hh, nh = shape.layers, shape.hidden, shape.heads
    dh = Hh // nh
    k0, k1 = obert.layer_keys(L - 2), obert.layer_keys(L - 1)
    pre = pre_rows(w, shape, ids, operand)
    if phantom is not None:
        pre = np.concatenate([pre, phantom[:1]])
    S = len(pre)
    g, b = f(k0["ln2_g"]), f(k0["ln2_b"])
    mean, inv = _stats(pre, shape.eps)
    x16 = r(pre)
    # step 1: the [CLS] query from the LayerNorm output of its row
    xcls = (x16[0] - mean[0]) * inv[0] * g + b
    Q = r(r(xcls) @ r(f(k1["q_w"])).T + f(k1["q_b"]))
    # the gain-folded K and V weights, their column sums and the folded bias (EPI_FOLD_F16's conventions)
    Wk, Wv = r(f(k1["k_w"]) * g), r(f(k1["v_w"]) * g)
    cs_v = Wv.sum(axis=1)
    c_v = f(k1["v_b"]) + f(k1["v_w"]) @ b
    # step 2
    u = r(np.stack([Q[h * dh:(h + 1) * dh] @ Wk[h * dh:(h + 1) * dh] for h in range(nh)]))  # [nh, H]
    if hooks.get("u_head_shift"):
        u = np.roll(u, 1, axis=0)
    alpha = u.sum(axis=1)  # = sum_c Q_c cs_k[c], over the values the products read
    # step 3
    shift = lambda a, d: a[np.clip(np.arange(S) + d, 0, S - 1)]  # noqa: E731
    inv_l = shift(inv, hooks.get("inv_shift", 0))
    mean_l = shift(mean, hooks.get("mean_shift", 0))
    dots = u @ x16.T  # [nh, S]
    s = inv_l[None] * (dots - (0.0 if hooks.get("no_mean_alpha") else mean_l[None] * alpha[:, None])) / math.sqrt(dh)
    keep = np.ones(S, bool)
    if "keys" in hooks:
        keep[:len(ids)] = hooks["keys"](len(ids))
    s = np.where(keep[None], s, -np.inf)
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p = p / p.sum(axis=1, keepdims=True)
    wt = r(p if hooks.get("no_inv_in_w") else p * inv_l[None])
    z = r(wt @ x16)  # [nh, H]
    gamma = wt @ mean_l
    # step 4
    ctx = np.concatenate([Wv[h * dh:(h + 1) * dh] @ z[h] - (0.0 if hooks.get("no_cs_gamma") else cs_v[h * dh:(h + 1) * dh] * gamma[h])
                          for h in range(nh)]) + c_v
    ctx = r(ctx)
    # the tail on the [CLS] row
    y = obert._ln(ctx @ r(f(k1["o_w"])).T + f(k1["o_b"]) + xcls, f(k1["ln1_g"]), f(k1["ln1_b"]), shape.eps)
    hdn = r(obert._gelu(r(y) @ r(f(k1["i_w"])).T + f(k1["i_b"])))
    return obert._ln(hdn @ r(f(k1["f_w"])).T + f(k1["f_b"]) + y, f(k1["ln2_g"]), f(k1["ln2_b"]), shape.eps)


# ---- planted mistakes: name -> (hooks, the lengths it touches) ------------------------------------------------------------
def _drop(idx):
    def keys(S):
        k = np.ones(S, bool)
        k[idx(S)] = False
        return k
    return keys


MISTAKES = {
    "last_key_dropped": ({"keys": _drop(lambda S: S - 1)}, lambda S: S >= 2),
    "key_0_dropped": ({"keys": _drop(lambda S: 0)}, lambda S: S >= 2),
    "group_dropped": ({"keys": _drop(lambda S: slice(CLS_GROUP * ((S - 1) // CLS_GROUP), S))}, lambda S: S > CLS_GROUP),
    "next_first_key_admitted": ("phantom", lambda S: True),
    "no_mean_alpha": ({"no_mean_alpha": True}, lambda S: S >= 2),
    "no_cs_gamma": ({"no_cs_gamma": True}, lambda S: True),
    "inv_from_next_row": ({"inv_shift": 1}, lambda S: S >= 2),
    "inv_from_previous_row": ({"inv_shift": -1}, lambda S: S >= 2),
    "mean_from_next_row": ({"mean_shift": 1}, lambda S: S >= 2),
    "mean_from_previous_row": ({"mean_shift": -1}, lambda S: S >= 2),
    "u_of_previous_head": ({"u_head_shift": True}, lambda S: S >= 2),  # (one key: its weight is 1 whatever the logit)
    "no_inv_in_weights": ({"no_inv_in_w": True}, lambda S: True),
}
# NOT COVERED: per head size, the (mistake, length) pairs at which the arithmetic leaves a mistake below 2 x TOL in these
# models. None at present beyond what the `touches` conditions above say (one key alone has weight 1 whatever its logit
# and statistics: S = 1 shows only what changes the value side); the thinnest margins are one key of MAX_POS (1.5-2.2 x
# the bar) and the mean term at S = 63, head size 64 (1.1 x). test_cls_collapse_cpu.py prints every margin and asserts all
# pairs not listed here.
NOT_COVERED = {64: (), 32: ()}


# ---- the models ---------------------------------------------------------------------------------------------------------
MEAN_PLANT = {64: 0.25, 32: 0.125}


class Model:
    def __init__(self, dh, seed=None):
        self.dh, self.heads = dh, H // dh
        self.shape = obert.BertShape(2, H, self.heads, I, vocab=VOCAB, max_pos=MAX_POS)
        w = obert.random_weights(self.shape, 8100 + dh if seed is None else seed)
        rng = np.random.default_rng(8200 + dh)
        k0, k1 = obert.layer_keys(0), obert.layer_keys(1)
        w[k0["o_w"]] = w[k0["o_w"]] * np.float32(0.25)  # layer 0 quiet: layer 1 still sees distinct tokens
        # layer 0's FFN-down: a mean (along 1) and a sigma (along a +-1 vector) that differ from token to token
        # (a mean of a few tenths of sigma: a larger one costs the f16 rows more bits than condition (c) allows, at
        # head size 32 sooner; a smaller one leaves the mean_j alpha_h term of one length of head size 64 below the bar)
        a, b2 = rng.normal(0, MEAN_PLANT[dh], I), rng.normal(0, 0.5, I)
        v = rng.choice([-1.0, 1.0], H)
        w[k0["f_w"]] = (np.outer(np.ones(H), a) + np.outer(v, b2)).astype(np.float32)
        w[k1["v_w"]] = w[k1["v_w"]] * np.float32(32.0)
        w[k1["o_w"]] = w[k1["o_w"]] * np.float32(32.0)
        for name in (k1["v_b"], k1["o_b"], k1["f_w"], k1["f_b"]):
            w[name] = np.zeros_like(w[name])
        self.w = {k: x.astype(np.float16).astype(np.float32) if x.ndim == 2 and "layer" in k else x for k, x in w.items()}
        self._rows = {}

    @property
    def name(self):
        return f"collapse-d{self.dh}"

    def cls_row(self, seq, **kw):
        return unit(collapsed_cls(self.w, self.shape, seq, **kw))

    def oracle_rows(self, seqs):
        return obert.sentence_embeddings(self.w, self.shape, seqs, "cls", True, np.float64)


_MODELS = {}


def model(dh):
    if dh not in _MODELS:
        _MODELS[dh] = Model(dh)
    return _MODELS[dh]


def engine(shape, w, pooling="cls", precision="f16", collapse=True, **over):
    """An engine with the model loaded; collapse False: loaded under VR_CLS_COLLAPSE=0 (read when a model is loaded)."""
    import os

    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    e = Engine(shape.hidden)
    desc = enc.BertDesc(shape.layers, shape.hidden, shape.heads, shape.intermediate, vocab=shape.vocab, max_pos=shape.max_pos,
                        type_vocab=shape.type_vocab, pooling=pooling, normalize=True, eps=shape.eps, precision=precision, **over)
    before = os.environ.get("VR_CLS_COLLAPSE")
    os.environ["VR_CLS_COLLAPSE"] = "1" if collapse else "0"
    try:
        enc.load_encoder(e, desc, w)
    finally:
        if before is None:
            del os.environ["VR_CLS_COLLAPSE"]
        else:
            os.environ["VR_CLS_COLLAPSE"] = before
    return e


def encode(e, seqs):
    from voitta_rag_amd import encoder as enc

    ids, off = pack(seqs)
    return enc.encode(e, ids, off)
