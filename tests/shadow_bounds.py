"""TEST INFRASTRUCTURE shared by test_shadow_bounds_cpu.py and test_shadow_bounds_gpu.py: an f64 restatement of the
two shadows of the two-stage dense search and of their error bounds, corpora whose planted rows use most of that bound,
and a catalogue of mistakes a kernel could make in its per-row words.

The model. Written from the formulas in the header comments of voitta_rag_amd/csrc/prefilter.hip and batch.hip
(every constant is listed in SOURCE_LINES with the source line it restates; test_shadow_bounds_cpu.py reads them back):
  int8   r = x - centre, s_r = max |r_i| / 127, r8 = clamp(rint(r / s_r), +-127), err_r = |r - s_r r8|_2 (rounded up);
         q = a qa + b qb + rho with a = max |q_i| / 127, b = a / 254;  A = s_r (a r8.qa + b r8.qb),
         E = err_r |q| + (1.001 + err_r) |rho| + c_fixed + 2e-6 s_r (|fa| + |fb|),  c_fixed = D 5e-7 max(|q|, 1) +
         1e-7 |q| sqrt(D) + |centre| |rho|.  The batched search charges the last term per query instead
         (2e-6 (2.01 + 2 |centre|) 1.25 |q|) and rounds its two regrouped constants up by 1.0000004.
  f16    h = f16(x), err_r = |x - h|_2 (rounded up); q = hi + lo (two f16);  A = h.(hi + lo),
         E = err_r |q| + c_fixed + 2e-7 |A|,  c_fixed = 1.001 (4.8e-7 |q| + 6e-8 sqrt(D)) + D 5e-7 max(|q|, 1).
  candidates = rows with A + E >= T, T = the k-th largest A - E among the live rows (single query) or among the best
         A - E of every 128-row slab (batched).
Scores are taken relative to the centre, f = (x - centre).q: the common term centre.q moves no comparison.
The centre the GPU sums with atomics cannot be reproduced to the bit, so the model only DESIGNS inputs and CAPS
candidate counts. The expected answer of every test is recomputed by oracle.core on the final corpus.

Planting (all on a background of unit Gaussian rows):
  starved winner      a row W that is badly represented in the shadow (int8: one component of 0.95, every other one
                      FRAC of a quantisation step, so they all round to 0; f16: components HALF of an f16 step off an
                      f16 value at the low end of a binade, four of them below the f16 normal range), asked with
                      q = normalise(x_W + LAMBDA * unit residual of W): W is rank 0 while its A underestimates f by most
                      of E. k dense decoys score a little below f_W. A bound that is too small for W drops it.
  inflated threshold  the mirror: k impostors whose residuals are parallel (one sign pattern) and a query ANTI-aligned
                      with it, so every impostor's A overestimates f by most of E; k dense winners score just above
                      them. A lower bound that is too high lifts T over the winners' upper bounds. The impostors share
                      their spike column: spikes at k different columns leave each an exact score of 0.95 |q_spike| <=
                      0.95 / sqrt(k), below the background's best row at k = 10 already.
  drifted centre      2,112 rows around a common direction, then 2,111 Gaussian rows quantised against the FIRST part's
                      centre (re-centring waits for the collection to double), then two more rows that cross the
                      doubling. (2,048 + 2,047 rows would stay below the 4,096 rows the two-stage search starts at.)

Every number below restates voitta_rag_amd/csrc; the geometry (tiles, scan blocks, slabs) is search_layouts'."""
import numpy as np

import search_layouts as sl
from oracle import core as ocore

FRAC = 0.45      # sub-step components of a spiky row, in quantisation steps (0.5 would round away from 0)
SPIKE = 0.95
LAMBDA = 2.0
REALISED_MIN = 0.8
CAND_CAP_SINGLE = 64
CAND_CAP_BATCHED = 256
CENTRE_MIN_ROWS = 1024  # prefilter.hip kCentreMinRows, api.hip `first + n >= 1024`

# (file, source text) of every constant the model uses
SOURCE_LINES = (
    ("prefilter.hip", "row_err[row] = sqrtf(e2) * 1.001f + 1.0e-12f;"),
    ("prefilter.hip", "const float s = finite ? mx / 127.0f : 0.0f;"),
    ("prefilter.hip", "fminf(fmaxf(rintf(x * inv), -127.0f), 127.0f)"),
    ("prefilter.hip", "sqrtf(e2) * 1.001f + 2.4e-7f * mx * sqrtf(static_cast<float>(dim)) + 1.0e-12f +"),
    ("prefilter.hip", "(centre ? 1.2e-7f * (1.001f + centre_norm) : 0.0f)"),
    ("prefilter.hip", "constexpr int64_t kCentreMinRows = 1024;"),
    ("prefilter.hip", "e->centre_norm = static_cast<float>(std::sqrt(n2) * 1.000001 + 1e-30);"),
    ("prefilter.hip", "const float qn = sqrtf(qn2) * 1.0001f + 1.0e-12f;"),
    ("prefilter.hip", "1.001f * (4.8e-7f * qn + 6.0e-8f * sqrtf(static_cast<float>(dim))) +"),
    ("prefilter.hip", "static_cast<float>(dim) * 5.0e-7f * fmaxf(qn, 1.0f);"),
    ("prefilter.hip", "const float err = ee[r] * qn + c_fixed + 2.0e-7f * fabsf(a);"),
    ("prefilter.hip", "const float b = a / 254.0f;"),
    ("prefilter.hip", "sqrtf(rho2_all) * 1.001f + 3.0e-7f * qn + 1.0e-12f"),
    ("prefilter.hip", "static_cast<float>(dim) * 5.0e-7f * fmaxf(qn, 1.0f) + 1.0e-7f * qn * sqrtf(static_cast<float>(dim)) +"),
    ("prefilter.hip", "centre_norm * rho_n;"),
    ("prefilter.hip", "ee[r] * qn + (1.001f + ee[r]) * rho_n + c_fixed + 2.0e-6f * ss[r] * (fabsf(fa) + fabsf(fb));"),
    ("batch.hip", "p[5] = 2.0e-6f * (2.01f + 2.0f * centre_norm) * 1.25f * qn;"),
    ("batch.hip", "p1 = (p[2] + p[3]) * 1.0000004f;"),
    ("batch.hip", "p2 = (1.001f * p[3] + p[4] + p[5]) * 1.0000004f;"),
    ("batch.hip", "err = fmaf(ee, p1, p2);"),
    ("batch.hip", "sqrtf(rho2_all) * 1.001f + 3.0e-7f * qn + 1.0e-12f"),
    ("api.hip", "first + n >= 1024 && first + n >= 2 * std::max(e->centre_rows, e->centre_checked_rows)"),
)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def prep(x):
    """the stored form of rows / the asked form of queries: oracle.core's cosine_preprocess, as f64"""
    x = np.ascontiguousarray(x, np.float32)
    return ocore.cosine_preprocess(x.reshape(-1, x.shape[-1])).astype(np.float64)


# ---- the engine's centre ----------------------------------------------------------------------------------------------

def centre_after(xh, upserts, centring=True):
    """The centre the int8 shadow is quantised against after each of the upserts (row counts), or None: the column
    mean of all rows stored when the collection reached 1,024 rows or doubled since the last attempt; a non-finite
    mean, or centring switched off, leaves no centre (and still counts as an attempt)."""
    centre, centre_rows, checked, n, out = None, 0, 0, 0, []
    for m in upserts:
        n += m
        if n >= CENTRE_MIN_ROWS and n >= 2 * max(centre_rows, checked):
            checked = n
            c = xh[:n].sum(0) / n if centring else None
            if c is not None and np.isfinite(c).all():
                centre, centre_rows = c, n
            else:
                centre, centre_rows = None, 0
        out.append(centre)
    return out


def rebuilt_centre(xh, centring=True):
    """after compact() or load(): the shadow is rebuilt around the column mean of the rows that are there"""
    return centre_after(xh, [xh.shape[0]], centring)[0]


# ---- the shadows --------------------------------------------------------------------------------------------------------

class Shadow:
    """form "int8": s [n], t [n, D] (the int8 values), res = r - s t, err [n]; form "f16": t = h, s = 1"""

    def __init__(self, form, xh, centre=None, clamp=True, scale_centre="same"):
        xh = np.asarray(xh, np.float64)
        self.form, self.xh, self.dim = form, xh, xh.shape[1]
        self.centre = None if centre is None else np.asarray(centre, np.float64)
        self.cn = 0.0 if centre is None else float(np.linalg.norm(self.centre) * 1.000001 + 1e-30)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if form == "f16":
                assert centre is None
                self.r = xh
                h = np.clip(xh.astype(np.float32), -65504.0, 65504.0).astype(np.float16).astype(np.float64)
                self.s, self.t, self.res = np.ones(xh.shape[0]), h, xh - h
                self.err = np.linalg.norm(self.res, axis=1) * 1.001 + 1e-12
                return
            self.r = r = xh if centre is None else xh - self.centre
            # scale_centre: the (mistaken) kernel takes the row's maximum from x - scale_centre, not from r
            r_scale = r if isinstance(scale_centre, str) else xh - np.asarray(scale_centre, np.float64)
            mx = np.abs(r_scale).max(1)
            finite = mx <= 3.0e38
            mx = np.where(finite, mx, 0.0)
            self.s = mx / 127.0
            t = np.rint(r * np.where(mx > 0, 127.0 / np.where(mx > 0, mx, 1.0), 0.0)[:, None])
            t = np.where(finite[:, None], t, 0.0)
            kept = np.clip(t, -127, 127)
            res = np.where(finite[:, None], r - self.s[:, None] * kept, 0.0)
            self.err = np.where(finite, np.linalg.norm(res, axis=1) * 1.001 + 2.4e-7 * mx * np.sqrt(self.dim) + 1e-12 +
                                (0.0 if centre is None else 1.2e-7 * (1.001 + self.cn)), np.inf)
            # without the clamp the byte that is stored is the low 8 bits of the integer
            self.t = kept if clamp else ((t.astype(np.int64) + 128) % 256 - 128).astype(np.float64)
            self.res = np.where(finite[:, None], r - self.s[:, None] * self.t, 0.0)

    def exact(self, qh):
        """f = (x - centre).q in f64"""
        return np.nan_to_num(self.r, nan=0.0, posinf=0.0, neginf=0.0) @ qh


class Bounds:
    pass


def bounds(sh, qh, batched=False, err=None, s=None, scale=1.0, drop=()):
    """A and E of every row for the preprocessed query qh. err, s: per-row words to use instead of the shadow's own
    (the catalogue's mistakes); scale: E multiplied; drop: terms of E left out ("err", "rho", "centre_rho")."""
    qh = np.asarray(qh, np.float64)
    err = sh.err if err is None else err
    s = sh.s if s is None else s
    d = sh.dim
    b = Bounds()
    qn = np.linalg.norm(qh) * 1.0001 + 1e-12
    err_term = 0.0 if "err" in drop else err * qn
    if sh.form == "f16":
        q32 = qh.astype(np.float32)
        hi = np.clip(q32, -65504.0, 65504.0).astype(np.float16)
        lo = (np.clip(q32, -65504.0, 65504.0) - hi.astype(np.float32)).astype(np.float16)
        b.A = sh.t @ (hi.astype(np.float64) + lo.astype(np.float64))
        c_fixed = 1.001 * (4.8e-7 * qn + 6.0e-8 * np.sqrt(d)) + d * 5.0e-7 * max(qn, 1.0)
        b.E = scale * (err_term + c_fixed + 2.0e-7 * np.abs(b.A))
        b.qn = qn
        return b
    t = np.abs(qh).max()
    ok = 0.0 < t <= 3.0e38
    a = t / 127.0 if ok else 0.0
    ta = np.clip(np.rint(qh * (127.0 / t if ok else 0.0)), -127, 127)
    r = qh - a * ta
    bq = a / 254.0
    tb = np.clip(np.rint(r * (254.0 / a if a > 0 else 0.0)), -127, 127)
    rho = r - bq * tb
    rho_n = np.linalg.norm(rho) * 1.001 + 3.0e-7 * qn + 1e-12 if ok else np.inf
    centre_rho = 0.0 if "centre_rho" in drop or "rho" in drop else sh.cn * rho_n
    c_fixed = d * 5.0e-7 * max(qn, 1.0) + 1.0e-7 * qn * np.sqrt(d) + centre_rho
    fa, fb = a * (sh.t @ ta), bq * (sh.t @ tb)
    b.A = s * (fa + fb)
    with np.errstate(invalid="ignore"):
        rho_term = 0.0 if "rho" in drop else (1.001 + err) * rho_n
        if batched:
            p5 = 2.0e-6 * (2.01 + 2.0 * sh.cn) * 1.25 * qn
            rho_row = 0.0 if "rho" in drop else err * rho_n
            rho_q = 0.0 if "rho" in drop else 1.001 * rho_n
            b.E = scale * 1.0000004 * (err_term + rho_row + rho_q + c_fixed + p5)
        else:
            b.E = scale * (err_term + rho_term + c_fixed + 2.0e-6 * s * (np.abs(fa) + np.abs(fb)))
    b.qn, b.rho_n = qn, rho_n
    return b


def candidates(b, k, mask=None, batched=False, widen=1.0, upper=None):
    """rows with A + E >= T. T: the k-th largest A - E of the live rows; batched: of the best A - E of every 128-row
    slab. Fewer than k in play: every live row. widen multiplies E (the cap the GPU's candidate count is held to).
    upper: the bounds the upper side is taken from when it is computed somewhere else than T (the batched search's
    revisit of the flagged tiles, batch_pairs_kernel, against the T of the scan)."""
    n = b.A.shape[0]
    live = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    u = b if upper is None else upper
    with np.errstate(invalid="ignore"):
        lo = np.where(live, b.A - widen * b.E, -np.inf)
        up = np.where(live, u.A + widen * u.E, -np.inf)
    lo = np.nan_to_num(lo, nan=-np.inf)
    up = np.where(np.isnan(up), np.inf, up)
    if batched:
        pad = -n % sl.SLAB_ROWS
        lo = np.concatenate([lo, np.full(pad, -np.inf)]).reshape(-1, sl.SLAB_ROWS).max(1)
    best = np.sort(lo[lo > -np.inf])[::-1]
    thr = best[k - 1] if best.shape[0] >= k else -3.0e38
    return np.flatnonzero(live & (up >= thr))


# ---- the catalogue of mistakes --------------------------------------------------------------------------------------------

def _shift(v, d):
    """word of row i + d in place of row i's; past either end of the array the model reads 0"""
    out = np.zeros_like(v)
    if d > 0:
        out[:-d] = v[d:]
    else:
        out[-d:] = v[:d]
    return out


# name -> bounds() arguments from the shadow; every one is a mistake in ONE per-row word or ONE term of E
ROW_WORD_MISTAKES = {
    "err_of_row+1": lambda sh: dict(err=_shift(sh.err, 1)),
    "err_of_row-1": lambda sh: dict(err=_shift(sh.err, -1)),
    "err_of_row+4": lambda sh: dict(err=_shift(sh.err, 4)),
    "err_of_row-4": lambda sh: dict(err=_shift(sh.err, -4)),
    "err_of_next_tile": lambda sh: dict(err=_shift(sh.err, sl.kTileRows)),
    "err_of_previous_tile": lambda sh: dict(err=_shift(sh.err, -sl.kTileRows)),
    "scale_of_row+1": lambda sh: dict(s=_shift(sh.s, 1)),
    "scale_of_row-1": lambda sh: dict(s=_shift(sh.s, -1)),
    "E_halved": lambda sh: dict(scale=0.5),
    "err_term_missing": lambda sh: dict(drop=("err",)),
}
F16_MISTAKES = tuple(m for m in ROW_WORD_MISTAKES if not m.startswith("scale_"))  # (the f16 shadow has no row scale)
# mistakes of the centre: they need the shadow of the OTHER centre, see stale_centre_mistakes()
CENTRE_MISTAKES = ("err_of_current_centre_bytes_of_old", "err_of_old_centre_bytes_of_current", "clamp_missing")
# NOT COVERED: at the planted gaps these leave the planted winners candidates in most or all cases; no test claims them
# (test_shadow_bounds_cpu.py prints which cases happen to see them)
NOT_COVERED = {
    "E_times_0.7": lambda sh: dict(scale=0.7),
    "rho_terms_missing": lambda sh: dict(drop=("rho",)),
    "centre_rho_term_missing": lambda sh: dict(drop=("centre_rho",)),
}

REVISIT_MISTAKE = "E_halved_in_the_revisit"  # batched only: T comes from the scan's (right) bounds, the upper side from half of E


def detects(case, sh, kwargs, mask=None, revisit_only=False):
    """a mistake counts as detected only if a planted winner (a row of the oracle's top k) leaves the candidate set"""
    b = bounds(sh, case.qh, batched=case.batched, **kwargs)
    if revisit_only:
        cand = candidates(bounds(sh, case.qh, batched=case.batched), case.k, mask, case.batched, upper=b)
    else:
        cand = candidates(b, case.k, mask, case.batched)
    return not np.isin(case.winners, cand).all()


# ---- planted cases ----------------------------------------------------------------------------------------------------------

class Case:
    """x (f32 corpus as upserted), q (f32 query), k, form, winners (planted rows that must be in the oracle's top k),
    planted (rows whose bound is used up), sign (+1: their A underestimates f, -1: overestimates), batched"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.qh = prep(self.q)[0]

    def shadow(self, centring=True):
        xh = prep(self.x)
        centre = rebuilt_centre(xh, centring) if self.form == "int8" else None
        return Shadow(self.form, xh, centre)

    def oracle_topk(self, mask=None):
        sc = sl.reference_scores(self.x, self.q)[0]
        return ocore.topk(sc, self.k, None if mask is None else np.asarray(mask, np.uint8))

    def realised(self, sh, b):
        """the smallest fraction of its E that a planted row realises"""
        f = sh.exact(self.qh)
        return float(np.min(self.sign * (f[self.planted] - b.A[self.planted]) / b.E[self.planted]))


def background(n, dim, seed):
    return unit(np.random.default_rng(seed).standard_normal((n, dim)))


def _scored_row(rng, qh, f):
    """a dense unit row with exact score f for the unit query qh"""
    u = rng.standard_normal(qh.shape[0])
    u = unit(u - (u @ qh) * qh)
    return f * qh + np.sqrt(1.0 - f * f) * u


def spiky_row(dim, centre, col, sign, pattern):
    """x = centre + beta r0, |x| = 1: r0 has SPIKE at col and pattern (in quantisation steps, |.| < 0.5) elsewhere, so
    against this centre every other component rounds to 0 and the whole pattern is the row's residual"""
    r0 = np.asarray(pattern, np.float64) * (SPIKE / 127.0)
    r0[col] = sign * SPIKE
    c = np.zeros(dim) if centre is None else centre
    qa, qb, qc = r0 @ r0, 2.0 * (c @ r0), c @ c - 1.0
    beta = (-qb + np.sqrt(qb * qb - 4.0 * qa * qc)) / (2.0 * qa)
    return c + beta * r0


HALF = 0.49  # of an f16 step: exactly 0.5 would leave the direction to the last bit of the row's normalisation


def halfway_row(rng, dim, signs=None, towards=None, where=None, steps=None):
    """a unit row whose components sit HALF of an f16 step from an f16 value at the low end of the binade
    [2^e, 2^(e+1)) nearest 1 / sqrt(D) from above (relative residual 2^-12 each, the most f16 allows), four more
    between two SUBNORMAL f16 values (absolute spacing 2^-24), and free components that bring the norm to 1.
    Rows that share (signs, towards, where, steps) have parallel residuals and differ in four of the f16 values they
    round to (one step each: their exact scores stay within a few hundredths of E of each other)."""
    e = int(np.ceil(np.log2(1.0 / np.sqrt(dim))))
    n_sub = 4
    n_half = min(dim - n_sub - max(8, dim // 16), int(0.93 * 2.0 ** (-2 * e)))
    if where is None:
        where = rng.permutation(dim)
        signs = rng.choice([-1.0, 1.0], dim)
        towards = rng.choice([-1.0, 1.0], dim)
        steps = rng.integers(1, 5, dim)
        mine = steps
    else:
        mine = steps.copy()
        mine[rng.choice(where[:n_half], 4, replace=False)] += 1
    half, sub, free = where[:n_half], where[n_half:n_half + n_sub], where[n_half + n_sub:]
    x = np.zeros(dim)
    x[half] = signs[half] * 2.0 ** e * (1.0 + (mine[half] + HALF * towards[half]) * 2.0 ** -10)
    x[sub] = signs[sub] * (rng.integers(2, 60, n_sub) + HALF * towards[sub]) * 2.0 ** -24
    x[free] = signs[free] * np.sqrt((1.0 - x @ x) / free.shape[0])
    return x, (signs, towards, where, steps)


def f16_lambda(dim, sigmas=4.6):
    """the largest weight of the residual direction that keeps f_W = 1 / sqrt(1 + lambda^2) at 4.6 sigma of the
    background's scores (sigma = 1 / sqrt(D)): more weight realises more of the bound"""
    return float(np.sqrt(dim / sigmas ** 2 - 1.0))


def f16_exact_row(row, qh=None, f=None):
    """The unit row `row` moved onto the f16 grid (err_r = 0: its E is c_fixed alone) with a sum of squares within
    3e-7 of 1, so that the keep rule of cosine_preprocess stores it as it is, and (with qh) an exact score within
    1e-6 of f: every component is rounded to f16, then single components are moved by one f16 step, always the move
    that brings (norm, score) closest. Dense companions of the f16 cases: a dense row's own f16 residual is a third of
    the largest possible one, too much for a neighbour's err_r or half of E to show."""
    v = np.asarray(row, np.float64).astype(np.float16).astype(np.float64)
    step = np.spacing(np.abs(v).astype(np.float16)).astype(np.float64)
    wf = 0.0 if qh is None else 1.0
    q = np.zeros_like(v) if qh is None else qh
    for _ in range(400):
        dn, df = v @ v - 1.0, (v @ q - f) if qh is not None else 0.0
        if abs(dn) <= 3e-7 and abs(df) <= 1e-6:
            break
        best = None
        for sgn in (1.0, -1.0):
            n2 = dn + 2.0 * sgn * v * step + step * step
            f2 = df + sgn * step * q
            cost = (n2 / 3e-7) ** 2 + wf * (f2 / 1e-6) ** 2
            j = int(np.argmin(cost))
            if best is None or cost[j] < best[0]:
                best = (cost[j], j, sgn)
        v[best[1]] += best[2] * step[best[1]]
        step[best[1]] = float(np.spacing(np.float16(abs(v[best[1]]))))
    out = v.astype(np.float32)
    assert np.array_equal(prep(out)[0], v) and np.array_equal(v.astype(np.float16).astype(np.float64), v), "not kept"
    return v


def f16_quiet_neighbours(x, rows, taken):
    """the rows 1, 4 and 16 before and after each of `rows` (those a mistaken index would read) made f16-exact"""
    for row in rows:
        for d in (-16, -4, -1, 1, 4, 16):
            if 0 <= row + d < x.shape[0] and row + d not in taken:
                x[row + d] = f16_exact_row(x[row + d])


def _rows_apart(n, count, first, stride):
    rows = first + stride * np.arange(count)
    assert rows.max() < n
    return rows


def plant_starved_winner(form, n, dim, k, w_row, seed=0, centring=True, lam=None, gaps=None, decoy_rows=None,
                         upserts=None, batched=False):
    """W at row w_row, rank 0 for q = normalise(x_W + lam * unit residual of W); k decoys at decoy_rows (default: one
    per 128-row slab, away from W's tile neighbours) score f_W - gaps * E_W (a linear ramp between the two fractions).
    upserts: the row counts of the appends that build the corpus (the centre W is designed against is the one its
    row is quantised with after the last of them)."""
    rng = np.random.default_rng(seed)
    x = background(n, dim, seed + 1)
    lam = lam or (LAMBDA if form == "int8" else f16_lambda(dim))
    # f16: c_fixed, a quarter of E_W, is never realised. Batched: the revisit alone may halve E while T stays right; W
    # then goes only if the k-th decoy's LOWER bound, gap + E_decoy below f_W, stays above f_W - (0.89 - 0.5) E_W
    gaps = gaps or ((0.05, 0.2) if form == "int8" and not batched else (0.02, 0.1))
    if decoy_rows is None:  # spread over the corpus, one per 128-row slab (the batched T_q counts a slab once) or,
        # when there are fewer slabs than decoys (single query only), one per 64 rows
        span = sl.SLAB_ROWS if batched or n // sl.SLAB_ROWS > k else 64
        free = np.setdiff1d(np.arange(n // span), [w_row // span])
        assert free.shape[0] >= k
        decoy_rows = free[np.linspace(0, free.shape[0] - 1, k).astype(np.int64)] * span + 37
    decoy_rows = np.asarray(decoy_rows, np.int64)
    assert w_row not in decoy_rows and np.abs(decoy_rows - w_row).min() > 2 * sl.kTileRows
    pattern = FRAC * rng.choice([-1.0, 1.0], dim)
    col, sign = int(rng.integers(dim)), 1.0
    proto = halfway_row(rng, dim)[0] if form == "f16" else None
    for _ in range(3):  # the centre moves a little with what is planted: design against it again
        xh = prep(x.astype(np.float32))
        centre = centre_after(xh, upserts or [n], centring)[-1] if form == "int8" else None
        x[w_row] = proto if form == "f16" else spiky_row(dim, centre, col, sign, pattern)
        xh = prep(x.astype(np.float32))
        sh = Shadow(form, xh[w_row:w_row + 1], centre)
        qh = unit(xh[w_row] + lam * unit(sh.res[0]))
        b = bounds(sh, qh, batched)
        f_w = xh[w_row] @ qh
        ramp = np.linspace(gaps[0], gaps[1], k) * b.E[0]
        for row, g in zip(decoy_rows, ramp):
            x[row] = _scored_row(rng, qh, f_w - g)
            if form == "f16":
                x[row] = f16_exact_row(x[row], qh, f_w - g)
    if form == "f16":
        f16_quiet_neighbours(x, [w_row] + decoy_rows.tolist(), set(decoy_rows.tolist()) | {w_row})
    return Case(x=x.astype(np.float32), q=qh.astype(np.float32), k=k, form=form, winners=np.array([w_row]),
                planted=np.array([w_row]), sign=1.0, batched=batched, decoys=decoy_rows, kind="starved")


def plant_inflated_threshold(form, n, dim, k, first_row, seed=0, centring=True, lam=None, gaps=None,
                             stride=sl.SLAB_ROWS, batched=False):
    """k impostors at first_row + stride * j with parallel residuals, asked with q = normalise(mean impostor -
    lam * unit mean residual): their A overestimates f. k dense winners, each three tiles behind an impostor, score
    the best impostor's f + gaps * the smallest impostor E (a linear ramp between the two fractions)."""
    rng = np.random.default_rng(seed)
    x = background(n, dim, seed + 1)
    lam = lam or (LAMBDA if form == "int8" else f16_lambda(dim, 5.0))  # (the anti-aligned part lowers f a little)
    gaps = gaps or ((0.02, 0.1) if form == "int8" else (0.01, 0.05))
    imp = _rows_apart(n, k, first_row, stride)
    win = imp + 3 * sl.kTileRows + 5  # three tiles on: no tile neighbour of an impostor
    assert win.max() < n
    pattern_sign = rng.choice([-1.0, 1.0], dim)
    col = int(rng.integers(dim))
    mags = FRAC * (1.0 - 0.25 * rng.random((k, dim)))  # distinct rows, one sign pattern
    shared = None
    protos = []
    for j in range(k):
        p, shared = halfway_row(rng, dim, *(shared or (None, None, None, None)))
        protos.append(p)
    for _ in range(3):
        xh = prep(x.astype(np.float32))
        centre = rebuilt_centre(xh, centring) if form == "int8" else None
        for j, row in enumerate(imp):
            x[row] = protos[j] if form == "f16" else spiky_row(dim, centre, col, 1.0, mags[j] * pattern_sign)
        xh = prep(x.astype(np.float32))
        sh = Shadow(form, xh[imp], centre)
        qh = unit(unit(xh[imp].mean(0)) - lam * unit(sh.res.mean(0)))
        b = bounds(sh, qh, batched)
        f = xh[imp] @ qh
        ramp = f.max() + np.linspace(gaps[0], gaps[1], k) * b.E.min()
        for row, fw in zip(win, ramp):
            x[row] = _scored_row(rng, qh, fw)
            if form == "f16":
                x[row] = f16_exact_row(x[row], qh, fw)
    if form == "f16":
        f16_quiet_neighbours(x, imp.tolist() + win.tolist(), set(imp.tolist()) | set(win.tolist()))
    return Case(x=x.astype(np.float32), q=qh.astype(np.float32), k=k, form=form, winners=win, planted=imp, sign=-1.0,
                batched=batched, kind="inflated")


# ---- row-word edges: where W goes ---------------------------------------------------------------------------------------------

def edge_rows(n):
    """name -> row of W: the 16 in-tile positions (of one tile in the middle of the corpus), the last partial tile, the
    first and last tile of a scan block's first visit, and a tile only the grid-stride walk reaches (when there is one)"""
    n_tiles, blocks = sl.scan_grid(n)
    slot, visit = sl.row_slots(n)
    mid = (blocks // 2) * sl.kScanWaves + 3
    rows = {f"pos{p}": mid * sl.kTileRows + p for p in range(sl.kTileRows)}
    if n % sl.kTileRows:
        rows["tail_last_row"] = n - 1
        rows["tail_first_row"] = n - n % sl.kTileRows
    b = blocks // 3
    rows["block_first_tile"] = b * sl.BLOCK_ROWS + 5
    rows["block_last_tile"] = b * sl.BLOCK_ROWS + (sl.kScanWaves - 1) * sl.kTileRows + 10
    strided = np.flatnonzero(visit >= sl.kTileRows)
    if strided.shape[0]:
        rows["grid_stride_tile"] = int(strided[min(7, strided.shape[0] - 1)])
    return rows


# ---- the drifted centre ---------------------------------------------------------------------------------------------------------

DRIFT_FIRST, DRIFT_SECOND, DRIFT_THIRD = 2112, 2111, 2


def anisotropic(rng, n, dim, cos, common):
    u = rng.standard_normal((n, dim))
    u = unit(u - (u @ common)[:, None] * common[None, :])
    return np.sqrt(cos) * common[None, :] + np.sqrt(1 - cos) * u


def drift_row(dim, centre_now, centre_other, col, sign):
    """A spiky unit row W for the centre mistakes: against centre_other every component of x - centre_other is a whole
    number of W's quantisation steps there (err_r ~ 0), against centre_now the same components are what is left of the
    drift between the two centres modulo a step (|.| <= half a step: they round to 0 or +-1 and err_r is that of a
    uniformly rounded row). A kernel that pairs the bytes of one centre with the err_r of the other has no bound for W."""
    x = np.zeros(dim)
    x[col] = sign * SPIKE
    others = np.arange(dim) != col
    for _ in range(8):
        step = abs(x[col] - centre_other[col]) / 127.0
        m = np.rint((centre_now - centre_other) / step)
        x[others] = (centre_other + step * m)[others]
        x[col] = sign * np.sqrt(1.0 - x[others] @ x[others])
    return x


def plant_drifted_centre(dim, k, seed=0, centring=True, stage="before"):
    """2,112 rows with pairwise cosine 0.7, then 2,111 Gaussian rows appended (quantised against the first part's
    centre), then 2 more rows that cross the doubling (everything re-quantised against the mean of all 4,225).
    W and its decoys live in the second part; W is designed against the centre of `stage` ("before" / "after" the
    doubling) and its spike points AGAINST that centre's largest component, so that its residual exceeds its own
    largest component. The same case object carries both questions: .upserts, and .asked = rows stored when asked."""
    rng = np.random.default_rng(seed)
    common = unit(rng.standard_normal(dim))
    n = DRIFT_FIRST + DRIFT_SECOND + DRIFT_THIRD
    upserts = [DRIFT_FIRST, DRIFT_SECOND, DRIFT_THIRD]
    x = np.concatenate([anisotropic(rng, DRIFT_FIRST, dim, 0.7, common), background(n - DRIFT_FIRST, dim, seed + 1)])
    asked = n - DRIFT_THIRD if stage == "before" else n
    w_row = DRIFT_FIRST + 1024 + 7
    slabs = np.arange(DRIFT_FIRST // sl.SLAB_ROWS + 1, (n - DRIFT_THIRD) // sl.SLAB_ROWS)
    slabs = slabs[slabs != w_row // sl.SLAB_ROWS]
    decoy_rows = slabs[np.linspace(0, slabs.shape[0] - 1, k).astype(np.int64)] * sl.SLAB_ROWS + 37
    pattern = FRAC * rng.choice([-1.0, 1.0], dim)
    for _ in range(3):
        xh = prep(x.astype(np.float32))
        centres = centre_after(xh, upserts, centring)
        centre, other = (centres[1], centres[2]) if stage == "before" else (centres[2], centres[1])
        col = int(np.argmax(np.abs(common)))
        sign = -np.sign(common[col])
        x[w_row] = spiky_row(dim, centre, col, sign, pattern) if centre is None else drift_row(dim, centre, other, col, sign)
        xh = prep(x.astype(np.float32))
        sh = Shadow("int8", xh[w_row:w_row + 1], centre)
        qh = unit(xh[w_row] + LAMBDA * unit(sh.res[0]))
        b = bounds(sh, qh)
        f_w = xh[w_row] @ qh
        for row, g in zip(decoy_rows, np.linspace(0.05, 0.2, k) * b.E[0]):
            x[row] = _scored_row(rng, qh, f_w - g)
    case = Case(x=x[:asked].astype(np.float32), q=qh.astype(np.float32), k=k, form="int8", winners=np.array([w_row]),
                planted=np.array([w_row]), sign=1.0, batched=False, decoys=decoy_rows, kind="drift-" + stage)
    case.all_rows, case.upserts, case.asked, case.stage = x.astype(np.float32), upserts, asked, stage
    return case


def drift_shadows(case, centring=True):
    """(shadow the engine holds when the case is asked, shadow of the same rows against the OTHER stage's centre)"""
    xh = prep(case.all_rows)
    c = centre_after(xh, case.upserts, centring)
    now, other = (c[1], c[2]) if case.stage == "before" else (c[2], c[1])
    rows = xh[:case.asked]
    return Shadow("int8", rows, now), Shadow("int8", rows, other)


def stale_centre_mistakes(case, centring=True):
    """({name: (shadow, bounds arguments)}, the shadow the engine holds) of the centre mistakes a drifted-centre case
    claims. The engine holds bytes, scales and errors of the centre of the case's stage.
      err_of_..._bytes_of_...   the bytes and scales stay, err_r comes from the OTHER centre's shadow (a stale row_err
                      kept across the re-centring, or one computed against a centre the bytes were not quantised with)
      clamp_missing   the row's scale is taken from max |x_i| (the row's own maximum) while the bytes hold x - centre,
                      and nothing clamps: W's spike, more than 127 steps, wraps around, and err_r (computed from the
                      unwrapped value) does not know. With the clamp the same scale is sound: err_r is exact for the
                      bytes that are stored. Only the clamp's absence, never the clamp alone, can be seen."""
    now, other = drift_shadows(case, centring)
    stale = "err_of_current_centre_bytes_of_old" if case.stage == "before" else "err_of_old_centre_bytes_of_current"
    wrapped = Shadow("int8", now.xh, now.centre, clamp=False, scale_centre=np.zeros(now.dim))
    honest = Shadow("int8", now.xh, now.centre, clamp=True, scale_centre=np.zeros(now.dim))
    out = {stale: (now, dict(err=other.err))}
    if case.stage == "after":  # (before the doubling |centre| is 0.84 and the same mistake wrecks most decoys as well:
        out["clamp_missing"] = (wrapped, dict(err=honest.err))  # T falls with them and W stays in, nothing to claim)
    return out, now


# ---- the shared case matrix -----------------------------------------------------------------------------------------------

N_TAIL15 = 4096 + 128 + 15
N_TAIL1 = 4096 + 128 + 1
N_BATCH = 16384 + 256 + 1
INT8_DIMS = (128, 384, 448)  # kb8n = 2 (tail loop only), 6 (exactly one unrolled group), 7 (group + tail)
F16_DIMS = (96, 256, 288)    # 96: the only form at that dim; 256, 288 with VR_PREFILTER=f16 (kb16n = 8: one group; 9: + tail)
# k = 64 needs W and 64 decoys, 65 candidates: over the cap of 64, which is not raised. 63 is the largest k that fits
# (inflated threshold: k impostors and k winners, so 32).
STARVED_K = (1, 10, 63)
INFLATED_K = (1, 10, 32)
W_MID = 2000


def _edges(form, dim, names):
    out = []
    for name in names:
        n = sl.N_GRID_STRIDE if name == "grid_stride_tile" else N_TAIL1 if name == "tail_one_row" else N_TAIL15
        row = n - 1 if name == "tail_one_row" else edge_rows(n)[name]
        out.append((f"{form}-d{dim}-starved-k10-{name}", dict(kind="starved", form=form, n=n, dim=dim, k=10, w_row=row)))
    return out


def single_cases(form):
    """[(name, arguments of plant())] of the single-query matrix of one shadow form"""
    out = []
    for dim in (INT8_DIMS if form == "int8" else F16_DIMS):
        for n, ks in ((N_TAIL15, STARVED_K), (N_TAIL1, (10,))):
            out += [(f"{form}-d{dim}-starved-n{n}-k{k}", dict(kind="starved", form=form, n=n, dim=dim, k=k, w_row=W_MID)) for k in ks]
        for n, ks in ((N_TAIL1, INFLATED_K), (N_TAIL15, (10,))):
            out += [(f"{form}-d{dim}-inflated-n{n}-k{k}", dict(kind="inflated", form=form, n=n, dim=dim, k=k, first_row=21, stride=64))
                    for k in ks]
        all_edges = [f"pos{p}" for p in range(sl.kTileRows)] + ["tail_last_row", "tail_first_row", "tail_one_row",
                                                                 "block_first_tile", "block_last_tile"]
        first = dim == (INT8_DIMS if form == "int8" else F16_DIMS)[0]
        out += _edges(form, dim, all_edges + (["grid_stride_tile"] if form == "int8" else []) if first else
                      ["pos3", "pos12", "tail_last_row"])
    return out


BATCH_DIMS = (128, 384)
_RB = 8  # a 256-row block in the middle of the batched corpus
BATCH_W_ROWS = {"first_slab": _RB * 256 + 5, "last_slab": _RB * 256 + 128 + 77, "partial_tile": N_BATCH - 1}


def batched_cases():
    out = []
    for dim in BATCH_DIMS:
        out += [(f"batched-d{dim}-starved-{name}", dict(kind="starved", form="int8", n=N_BATCH, dim=dim, k=10, w_row=row, batched=True))
                for name, row in BATCH_W_ROWS.items()]
        out.append((f"batched-d{dim}-inflated", dict(kind="inflated", form="int8", n=N_BATCH, dim=dim, k=10, first_row=21, batched=True)))
    return out


def plant(centring=True, **kw):
    """the case of the matrix that single_cases() / batched_cases() describe with these arguments"""
    kind = kw.pop("kind")
    fn = plant_starved_winner if kind == "starved" else plant_inflated_threshold
    return fn(kw.pop("form"), kw.pop("n"), kw.pop("dim"), kw.pop("k"), centring=centring, **kw)


# The int8 cases realise 0.8 of E and more. An f16 row cannot: c_fixed, the allowance for the two f32 accumulation chains
# (D 5e-7), is no input's to realise and is a tenth of the largest possible E at D = 96, a quarter at D = 256 and 288.
# Floors of the f16 form: the smallest fraction any case of that (dim, kind) reaches in the model, minus 0.05
# (profiles/shadow_bounds_checks.md has the fractions).
REALISED_FLOOR_F16 = {(96, "starved"): 0.8, (96, "inflated"): 0.70, (256, "starved"): 0.70, (256, "inflated"): 0.66,
                      (288, "starved"): 0.68, (288, "inflated"): 0.66}


def realised_floor(case):
    return REALISED_MIN if case.form == "int8" else REALISED_FLOOR_F16[(case.x.shape[1], case.kind)]


def required_mistakes(case):
    """the catalogue entries a case must detect: a starved winner every row word; an inflated threshold those of err_r
    and E (a neighbour's scale moves the impostors' A either way)"""
    names = ROW_WORD_MISTAKES if case.form == "int8" else F16_MISTAKES
    return [m for m in names if case.kind == "starved" or not m.startswith("scale_")]


def check_case(case, centring=True, mask=None):
    """the four model checks of a planted case -> (realised fraction, candidates, undetected required mistakes)"""
    sh = case.shadow(centring)
    b = bounds(sh, case.qh, case.batched)
    cand = candidates(b, case.k, mask, case.batched)
    missed = [m for m in required_mistakes(case) if not detects(case, sh, ROW_WORD_MISTAKES[m](sh), mask)]
    if case.batched and case.kind == "starved" and not detects(case, sh, dict(scale=0.5), mask, revisit_only=True):
        missed.append(REVISIT_MISTAKE)
    return case.realised(sh, b), cand, missed
