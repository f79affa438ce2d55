"""TEST INFRASTRUCTURE shared by test_sparse_layouts_cpu.py and test_sparse_layouts_gpu.py: sparse corpora whose winners
sit where the inverted-index routes (voitta_rag_amd/csrc/invert.hip) are least comfortable, and a CPU model of the route
each call then takes.

Corpora. A corpus is assembled from LAYERS, as vectorised CSR arrays (no Python loop over rows): a background layer (a
Zipfian vocabulary, what the riders of a batch ask for) and, per planted case, a few term ids of its own with chosen
document frequencies (hence chosen IDF weights). A planted layer is written in canonical order (entry j = the j-th
best value) and PLACED by a position array, the dense file's planting by permutation: which rows carry the term, hence
which segment, which 512-row wave slice and which posting position a winner occupies; neither a df nor a score depends on
it. The expected answer of a test is always recomputed by oracle.core on the assembled corpus, never taken from the plan.

Route model. From the oracle's scores, the document frequencies and the segment table alone (the upsert sizes give the
segments) the model states which SparseRoute a call takes, which segments the sample reads, how many sample keys a query
gets and hence whether it has a threshold, how many rows of each segment reach it, whether a region spills and whether
the query is redone; for the per-query route the seed's essential terms and, per block, the non-essential terms and the
"worth it" rule. The grouped route compares integer keys (exact: the model reproduces it to the key); the per-query
route's bounds carry rounding slack (* 1.000001f, * 1.00001f), which the model does NOT reproduce: every inequality it
relies on is returned with its margin, and the planted cases keep each margin above MARGIN = 1 %.

Every number below restates a constant of voitta_rag_amd/csrc (test_sparse_layouts_cpu.py reads them back):
  kInvSegRows      = 4096  engine_internal.h  rows of a segment, at most
  kInvMaxTerms     = 32    engine_internal.h  distinct terms of a query the inverted scan takes (more: the forward scan)
  kScanBlocks      = 512   engine_internal.h  blocks per query of the per-query scans, at most
  kListLen         = 64    topk_device.h      entries of a wave's list: k <= 64
  kInvWaves        = 4     invert.hip         waves of a per-query block
  kInvMaxSurvivors = 1024  invert.hip         rows of a segment inv_scan_segments scores one by one (beyond: the full sum)
  kPrunedCand      = 512   invert.hip         candidate rows a wave of sparse_inv_pruned_kernel buffers
  kPrunedHash      = 1024  invert.hip         slots of its table of partial sums; 3/4 full passes the rest on unfiltered
  kSeedStride      = 4     invert.hip         the seed pass reads every fourth segment
  kSeedRowsPerWave = 1024  invert.hip         ... and a wave scores at most this many rows
  kGrpThreads      = 512   invert.hip         threads of a grouped block: 8 waves, 8 rows per thread
  kGrpMaxU         = 64    invert.hip         union terms of a group
  kGrpCandCap      = 16    invert.hip         keys per (query, segment) region, at least
  kSampleTail      = 4     invert.hip         last segments the sample always reads
  GROUP = 2, SPILL = 4096, SELECT_KEYS = 1024 * 8 (topk.hip, select_regions_kernel<1024, 8>), GROUPED_MIN_QUERIES = 16,
  SAMPLED_MIN_SEGMENTS = 128, region_cap() = inv_region_cap, rebuilds() = inv_append's rebuild rule."""
import numpy as np

from oracle import core as ocore
from search_layouts import make_keys

kInvSegRows = 4096
kInvMaxTerms = 32
kScanBlocks = 512
kListLen = 64
kInvWaves = 4
kInvMaxSurvivors = 1024
kPrunedCand = 512
kPrunedHash = 1024
kSeedStride = 4
kSeedRowsPerWave = 1024
kGrpThreads = 512
kGrpMaxU = 64
kGrpCandCap = 16
kSampleTail = 4

CONSTANT_SOURCES = {
    "kInvSegRows": "engine_internal.h", "kInvMaxTerms": "engine_internal.h", "kScanBlocks": "engine_internal.h",
    "kListLen": "topk_device.h", "kInvWaves": "invert.hip", "kInvMaxSurvivors": "invert.hip", "kPrunedCand": "invert.hip",
    "kPrunedHash": "invert.hip", "kSeedStride": "invert.hip", "kSeedRowsPerWave": "invert.hip", "kGrpThreads": "invert.hip",
    "kGrpMaxU": "invert.hip", "kGrpCandCap": "invert.hip", "kSampleTail": "invert.hip",
}

GROUP = 2                      # queries per grouped block (inv_scan_grouped: kGroup)
SPILL = 4096                   # keys of a query's spill area (kSpillCap's default)
SELECT_KEYS = 1024 * 8         # keys select_regions_kernel ranks per query; more: the query is redone
GROUPED_MIN_QUERIES = 16       # inv_grouped_fits: nq >= 16
SAMPLED_MIN_SEGMENTS = 128     # inv_pick_route: n_inv_seg >= 128
SAMPLE_REGULAR = 16            # seg_stride = n_seg / 16
SLICE_ROWS = kGrpThreads // 64 * 8 * 8  # 512: the rows of a segment one wave of a grouped block looks at
PRUNED_TABLE_ROWS = kPrunedHash * 3 // 4  # 768: postings after which a wave's table passes rows on unfiltered
PRUNED_FLUSH = kPrunedCand - 64           # 448: buffered candidates beyond which the next 64 force a flush
MARGIN = 0.01

ROUTE_FULL, ROUTE_SEED_PRUNED, ROUTE_GROUPED_SEED, ROUTE_GROUPED_SAMPLED = "kFull", "kSeedPruned", "kGroupedSeed", "kGroupedSampled"


# ---- segments -------------------------------------------------------------------------------------------------------

def region_cap(n_seg):
    """inv_region_cap: keys of a (query, segment) region"""
    return max(kGrpCandCap, min(512, 8192 // max(n_seg, 1)))


def rebuilds(upserts):
    """The upserts (1-based) at which inv_append sorts the whole collection into full segments again: more than 64
    segments and more than 4 x ceil(rows / 4096) of them."""
    out, n_seg, rows = [], 0, 0
    for i, n in enumerate(upserts):
        n_seg += -(-n // kInvSegRows)
        rows += n
        if n_seg > 64 and n_seg > 4 * -(-rows // kInvSegRows):
            out.append(i + 1)
            n_seg = -(-rows // kInvSegRows)
    return out


def segment_table(upserts):
    """(row_base, nrows) of every segment, in order: an upsert of n rows becomes n_sub = ceil(n / 4096) segments of
    seg_rows = ceil(n / n_sub) rows (the last one what is left). Only for upsert sequences that never rebuild."""
    assert not rebuilds(upserts)
    base, rows, at = [], [], 0
    for n in upserts:
        n_sub = -(-n // kInvSegRows)
        seg_rows = -(-n // n_sub)
        for j in range(n_sub):
            base.append(at + j * seg_rows)
            rows.append(min(seg_rows, n - j * seg_rows))
        at += n
    return np.array(base, np.int64), np.array(rows, np.int64)


def sampled_segments(n_seg):
    """The segments the sample pass reads: every seg_stride-th (seg_stride = n_seg / 16), then the last kSampleTail."""
    stride = n_seg // SAMPLE_REGULAR
    n_samp = (n_seg - kSampleTail + stride - 1) // stride + kSampleTail
    n_regular = n_samp - kSampleTail
    return [y * stride for y in range(n_regular)] + [n_seg - (n_samp - y) for y in range(n_regular, n_samp)]


def segment_of(rows, seg_base):
    return np.searchsorted(seg_base, np.asarray(rows), side="right") - 1


# ---- routes ---------------------------------------------------------------------------------------------------------

def pick_route(nq, n_seg, weights_given=False, grouped_env=True, sample_env=True, allow_grouped=True):
    """inv_pick_route for a batch with a host CSR (every batch the C-ABI takes). grouped_env / sample_env False:
    VR_SPARSE_GROUPED=0 / VR_SPARSE_GROUP_SAMPLE=0. allow_grouped False: the redo of overflowed queries."""
    if weights_given:
        return ROUTE_FULL
    fits = nq >= GROUPED_MIN_QUERIES and n_seg <= 65535 and nq * n_seg * region_cap(n_seg) <= 1 << 28
    if not (allow_grouped and grouped_env and fits):
        return ROUTE_SEED_PRUNED
    return ROUTE_GROUPED_SAMPLED if n_seg >= SAMPLED_MIN_SEGMENTS and sample_env else ROUTE_GROUPED_SEED


def blocks_per_query(nq, n_seg, env_blocks=None):
    """gx of inv_scan_topk_batch (VR_SPARSE_BATCH_BLOCKS = env_blocks) and gs, the seed pass's blocks per query"""
    gx = min(n_seg, max(1, (16384 + nq - 1) // nq))
    if env_blocks is not None:
        gx = min(n_seg, max(1, env_blocks))
    gx = min(gx, kScanBlocks)
    return gx, min(gx, 16)


def grouped_prepare(scores, passing, seg_base, seg_rows):
    """What grouped_model needs of one query whatever k is: its ranking keys and its sample keys, best first (per sampled
    segment the best key of each 512-row slice; 0 where a slice holds no row that passes and shares a term)."""
    keys = make_keys(scores, passing)
    samp = []
    for s in sampled_segments(seg_base.shape[0]):
        seg = keys[seg_base[s]:seg_base[s] + seg_rows[s]]
        samp += [seg[a:a + SLICE_ROWS].max() for a in range(0, seg.shape[0], SLICE_ROWS)]
    return keys, np.sort(np.array(samp, np.uint64))[::-1]


def grouped_model(scores, passing, k, seg_base, seg_rows, sampled=True, threshold_key=None, prep=None):
    """What the grouped scan does with ONE query, from its oracle scores (-inf: the row shares no term), the rows that
    pass (live and filter) and the segment table. Integer keys throughout, as in the kernel: exact.
    sampled: the threshold is the k-th best of the sample keys; fewer than k sample keys: no threshold, every row the
    query touches is offered. Otherwise threshold_key is given (the seed's k-th key, or 0). prep: grouped_prepare's
    result for these scores (shared between the k of a test).
    -> dict: sample_keys, threshold (key, 0 = none), offered[seg], spilled, gathered (keys the selection ranks: what
    sparse_group_candidates counts), redo."""
    n_seg = seg_base.shape[0]
    keys, samp = prep if prep is not None else grouped_prepare(scores, passing, seg_base, seg_rows)
    out = {"sample_keys": None}
    if sampled:
        n_keys = int(np.count_nonzero(samp))
        out["sample_keys"] = n_keys
        threshold_key = samp[k - 1] if n_keys >= k else np.uint64(0)
    th = np.uint64(threshold_key or 0)
    reach = (keys != 0) & (keys >= th)
    offered = np.add.reduceat(reach.astype(np.int64), seg_base)
    cap = region_cap(n_seg)
    spilled = int(np.maximum(offered - cap, 0).sum())
    gathered = int(np.minimum(offered, cap).sum()) + min(spilled, SPILL)
    out.update(threshold=int(th), offered=offered, spilled=spilled, gathered=gathered,
               redo=spilled > SPILL or gathered > SELECT_KEYS)
    return out


def key_score(key):
    """the f32 score inside a ranking key (inv_key_score)"""
    hi = np.uint32(int(key) >> 32)
    bits = hi ^ np.uint32(0x80000000) if hi & np.uint32(0x80000000) else ~hi
    return float(np.array([bits], np.uint32).view(np.float32)[0])


# ---- the per-query route: seed, then blocks that prune or hand their share over ---------------------------------------

def query_weights(oracle, q_idx, q_val):
    """(ids ascending, weights q * idf, fractions df / N) of a query as the engine forms them (a repeated id keeps its
    first value); the idf is the oracle's."""
    first = {}
    for i, v in zip(np.asarray(q_idx).tolist(), np.asarray(q_val, np.float32).tolist()):
        first.setdefault(int(i), v)
    ids = np.array(sorted(first), np.int32)
    df = np.array([oracle.df.get(int(i), 0) for i in ids], np.int64)
    w = np.array([np.float32(first[int(i)]) * np.float32(ocore.idf(oracle.n_points, int(d))) for i, d in zip(ids, df)], np.float32)
    return ids, w, np.minimum(df / np.float32(oracle.n_points), 1.0)


def term_order(w):
    """t_ord: term indices by ascending |weight| (ties: by index) and the running sums t_pre (not rounded up)"""
    order = np.argsort(np.abs(w), kind="stable")
    return order, np.cumsum(np.abs(w[order]).astype(np.float64))


def seed_essential(w, frac, n_points, k):
    """The seed pass's choice: the terms of largest |weight| until they are expected to name max(4 k, 64) rows of the
    quarter of the segments it reads. -> (ne, margin): t_ord[ne:] are essential (ne = None: no seed: no term names a
    row); margin = the relative distance of the deciding sums from `want`, on the tighter side."""
    order, _ = term_order(w)
    want = max(4.0 * k, 64.0)
    rows, margin = 0.0, np.inf
    for j in range(len(w) - 1, -1, -1):
        before = rows
        rows += float(frac[order[j]]) * n_points / kSeedStride
        if rows >= want:
            margin = min(rows / want - 1.0, 1.0 - before / want if j < len(w) - 1 else np.inf)
            return j, margin
    if rows > 0.0:
        return 0, 1.0 - rows / want
    return None, np.inf


def block_prunes(w, frac, theta, vmax):
    """sparse_inv_pruned_kernel<false>, one block: theta = the seed's k-th score, vmax = the largest |weight| of the
    block's segments. -> (n_ne, prunes, margin): the terms t_ord[:n_ne] are non-essential (t_pre * vmax < theta); the
    block prunes iff n_ne > 0 and ess * 3 < all and ess < 0.15 (document-frequency shares), else it flags need_full.
    margin: the smallest relative distance of any of these inequalities from equality."""
    order, pre = term_order(w)
    margins = []
    n_ne = 0
    if theta is not None and theta > 0:
        bound = pre * float(vmax)
        n_ne = int(np.count_nonzero(bound < theta))  # (the sums only grow: a prefix)
        margins += [abs(b / theta - 1.0) for b in bound]
    if n_ne == 0:
        return 0, False, min(margins, default=np.inf)
    f = np.asarray(frac, np.float64)[order]
    ess, total = f[n_ne:].sum(), f.sum()
    ok = ess * 3.0 < total and ess < 0.15
    margins += [abs(ess * 3.0 / total - 1.0), abs(ess / 0.15 - 1.0)]
    return n_ne, bool(ok), min(margins)


def share_of_block(n_seg, gx, bx):
    """the segments block bx of gx walks in the pruned and the full scan: bx, bx + gx, ...; wave w of a pruned block takes
    every kInvWaves-th of them from the w-th on"""
    return list(range(bx, n_seg, gx))


# ---- corpora --------------------------------------------------------------------------------------------------------

BACKGROUND_TERM0, BACKGROUND_STEP = 100_000, 7   # background vocabulary ids: above every planted term


def background_layer(n, vocab, per_row, seed):
    """A Zipfian vocabulary: per_row draws per row (p ~ 1 / rank^1.1), duplicates dropped; values in [0.2, 2.2)."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocab + 1) ** 1.1
    t = rng.choice(vocab, size=(n, per_row), p=p / p.sum())
    pair = np.unique(np.arange(n, dtype=np.int64)[:, None] * vocab + t)
    rows, terms = pair // vocab, (pair % vocab).astype(np.int32) * BACKGROUND_STEP + BACKGROUND_TERM0
    return rows, terms, rng.uniform(0.2, 2.2, size=rows.shape[0]).astype(np.float32)


def background_terms(vocab):
    return np.arange(vocab, dtype=np.int32) * BACKGROUND_STEP + BACKGROUND_TERM0


def planted_layer(term, values, positions):
    """Term `term` with value values[j] on row positions[j] (distinct rows): rank j of the plan sits at positions[j]."""
    positions = np.asarray(positions, np.int64)
    values = np.asarray(values, np.float32)
    assert positions.shape == values.shape and np.unique(positions).shape[0] == positions.shape[0]
    return positions, np.full(positions.shape[0], term, np.int32), values


def assemble(n, layers):
    """CSR (off int64, idx int32, val f32) of n rows from (rows, terms, values) layers; every row sorted by term id; no
    row lists a term twice (asserted: such collections leave the inverted index)."""
    rows = np.concatenate([np.asarray(l[0], np.int64) for l in layers])
    terms = np.concatenate([np.asarray(l[1], np.int32) for l in layers])
    vals = np.concatenate([np.asarray(l[2], np.float32) for l in layers])
    assert rows.min() >= 0 and rows.max() < n and terms.min() >= 0
    o = np.lexsort((terms, rows))
    rows, terms, vals = rows[o], terms[o], vals[o]
    assert not np.any((rows[1:] == rows[:-1]) & (terms[1:] == terms[:-1]))
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=off[1:])
    return off, terms, vals


def spread(seg_base, seg_rows, segments, per_segment, start=3, step=None):
    """per_segment rows in each of `segments`, evenly stepped through the segment from row `start` (both 512-row slices
    of a 1024-row segment get their share)"""
    out = []
    for s in segments:
        st = step or max(1, (int(seg_rows[s]) - start) // per_segment)
        r = seg_base[s] + start + st * np.arange(per_segment)
        out.append(r[r < seg_base[s] + seg_rows[s]])  # (a one-row segment takes none)
    return np.concatenate(out)


def riders(nq, vocab, seed, max_terms=8):
    """nq queries over the background vocabulary (Zipfian: they share their common terms), weights in [0.5, 1.5)"""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocab + 1) ** 1.1
    ids = background_terms(vocab)
    out = []
    for _ in range(nq):
        m = int(rng.integers(1, max_terms + 1))
        out.append((np.sort(rng.choice(ids, size=m, replace=False, p=p / p.sum())).astype(np.int32),
                    rng.uniform(0.5, 1.5, size=m).astype(np.float32)))
    return out


def group_queries(qs, G=GROUP):
    """inv_group_queries: the batch's queries (<= kInvMaxTerms distinct terms, not empty) ordered by the (-frequency in the
    batch, id) of their three commonest terms, then cut into groups of <= G whose union of terms stays <= kGrpMaxU.
    -> [(members, union size)]"""
    ids = [np.unique(q[0]) for q in qs]
    served = [i for i, t in enumerate(ids) if 0 < t.shape[0] <= kInvMaxTerms]
    freq = {}
    for i in served:
        for t in ids[i].tolist():
            freq[t] = freq.get(t, 0) + 1
    def key(i):
        top = sorted((-freq[t], t) for t in ids[i].tolist())[:3]
        flat = [v for pair in top for v in pair]
        return flat + [0] * (6 - len(flat)) + [i]
    groups, members, uni = [], [], np.zeros(0, np.int32)
    for i in sorted(served, key=key):
        merged = np.union1d(uni, ids[i])
        if members and (len(members) >= G or merged.shape[0] > kGrpMaxU):
            groups.append((members, uni.shape[0]))
            members, merged = [], ids[i]
        uni = merged
        members = members + [i]
    if members:
        groups.append((members, uni.shape[0]))
    return groups


# ---- geometry S: three engines over one family of corpora ------------------------------------------------------------

VOCAB = 300
GEOMETRIES = {
    "s1024": [1024] * 128,           # 131,072 rows, 128 segments: 2 sample keys x 20 sampled segments = 40 at most
    "s1021": [1021] * 133,           # segment bases that are no multiple of 8 or 32; 21 sampled segments, 128 next to 129..132
    "s1row": [1024] * 128 + [1],     # 129 segments, the last one a single row (nrows = 1, partial pass8); one row fewer
                                     # and the 129th segment would trigger the rebuild (129 > 4 * 32)
    "p4096": [5 * 4096],             # one upsert: 5 full segments (geometry P)
}

# planted term ids (all below the background's)
T_INVISIBLE, T_ONLY64, T_ONLY65, T_FLOOD, T_TAIL, T_LAST, T_NEAR, T_TIE = 11, 23, 24, 25, 31, 32, 33, 41
T_POS, T_NEG, T_CANCEL_A, T_CANCEL_B, T_ALLNEG, T_ABSENT, T_FIRSTROW = 51, 52, 53, 54, 55, 61, 71
T_LONG0 = 1000  # 64 terms for the long queries: T_LONG0 + j
T_SURV = (81, 82, 83)   # geometry P: essential terms naming 1023 / 1024 / 1025 rows of one segment
T_BALLAST = 96           # geometry P: a term every row carries (pure non-essential ballast)
TIE_GROUP = 70


def unsampled(n_seg):
    s = set(sampled_segments(n_seg))
    return [i for i in range(n_seg) if i not in s]


def corpus_s(name):
    """(off, idx, val, folder, plan) of geometry `name`: the background plus every planted layer of the S cases. plan:
    what the tests need to know about the layers (rows of the tie group, ...). Folders: 0 for most rows, see below."""
    ups = GEOMETRIES[name]
    n = sum(ups)
    base, rows = segment_table(ups)
    n_seg = base.shape[0]
    samp, uns = sampled_segments(n_seg), unsampled(n_seg)
    rng = np.random.default_rng(sum(map(ord, name)))
    layers = [background_layer(n, VOCAB, 6, 17)]
    plan = {"n": n, "seg_base": base, "seg_rows": rows, "n_seg": n_seg}
    # winners invisible to the sample: 64 strong rows (distinct values 3.0 .. 2.37) in segments 1..7, and six weak rows
    # (values <= 0.5) in EVERY segment, three per 512-row slice: the sample sees only weak rows, but a full list of them
    strong = spread(base, rows, range(1, 8), 10, start=5)[:64]
    weak = spread(base, rows, range(n_seg - (name == "s1row")), 6, start=1)
    weak = np.setdiff1d(weak, strong)
    layers.append(planted_layer(T_INVISIBLE, np.concatenate([3.0 - 0.01 * np.arange(64), rng.uniform(0.1, 0.5, weak.shape[0])]),
                                np.concatenate([strong, weak])))
    plan["invisible_strong"] = strong
    # terms that occur only in unsampled segments: 64 rows of one segment, 65 of another, 150 rows in each of 49
    layers.append(planted_layer(T_ONLY64, rng.uniform(0.5, 2.0, 64), spread(base, rows, [uns[2]], 64, start=2)))
    layers.append(planted_layer(T_ONLY65, rng.uniform(0.5, 2.0, 65), spread(base, rows, [uns[4]], 65, start=0)))
    flood_segs = uns[10:59]
    layers.append(planted_layer(T_FLOOD, rng.uniform(0.5, 2.0, 49 * 150), spread(base, rows, flood_segs, 150, start=1)))
    plan["flood_segments"] = flood_segs
    # winners only in the tail segments (which the sample always reads); only in the last segment
    layers.append(planted_layer(T_TAIL, rng.uniform(0.5, 2.0, 4 * 30), spread(base, rows, range(n_seg - 4, n_seg - 1), 40, start=7)))
    # next to the tail: the two best rows in the two slices of segment n_seg - 5 (on 133 x 1021 the LAST regular sample,
    # right before the tail: a tail that began one segment too low would read it twice), ten lower rows in the first tail segment
    near = np.concatenate([base[n_seg - 5] + np.array([100, 700]), spread(base, rows, [n_seg - 4], 10, start=3)])
    layers.append(planted_layer(T_NEAR, np.concatenate([[2.5, 2.4], 1.5 - 0.05 * np.arange(10)]), near))
    last_rows = np.arange(base[-1], base[-1] + min(rows[-1], 12))
    layers.append(planted_layer(T_LAST, 2.0 - 0.1 * np.arange(last_rows.shape[0]), last_rows))
    # a tie group: 70 rows with the SAME value, half of them in sampled segments, half in unsampled ones; 200 lower rows
    tie = np.concatenate([spread(base, rows, samp[2:9], 5, start=9), spread(base, rows, uns[60:67], 5, start=11)])
    assert tie.shape[0] == TIE_GROUP
    low = spread(base, rows, uns[70:90], 10, start=13)
    layers.append(planted_layer(T_TIE, np.concatenate([np.full(TIE_GROUP, 1.75), rng.uniform(0.2, 1.0, low.shape[0])]),
                                np.concatenate([tie, low])))
    plan["tie_rows"] = np.sort(tie)
    # mixed signs. T_POS x T_NEG: rows with only T_NEG score negative; 100 rows carry T_CANCEL_A and T_CANCEL_B with the
    # same value, so a query (+w, -w) on two terms of EQUAL df sums them to exactly +0.0; T_ALLNEG for an all-negative query
    pos = spread(base, rows, samp[:5] + uns[:10], 3, start=17)
    neg = spread(base, rows, samp + uns[20:40], 4, start=19)  # both slices of every sampled segment: a full sample list
    layers.append(planted_layer(T_POS, rng.uniform(0.5, 2.0, pos.shape[0]), pos))
    layers.append(planted_layer(T_NEG, rng.uniform(0.5, 2.0, neg.shape[0]), neg))
    both = spread(base, rows, samp[3:8] + uns[40:45], 10, start=23)
    only_a = spread(base, rows, samp[8:12] + uns[45:51], 3, start=29)   # negative rows
    only_b = spread(base, rows, samp[12:16] + uns[51:57], 3, start=31)  # positive rows: 30, fewer than k = 64
    v = rng.uniform(0.5, 2.0, both.shape[0])
    layers.append(planted_layer(T_CANCEL_A, np.concatenate([v, rng.uniform(0.5, 2.0, only_a.shape[0])]), np.concatenate([both, only_a])))
    layers.append(planted_layer(T_CANCEL_B, np.concatenate([v, rng.uniform(0.5, 2.0, only_b.shape[0])]), np.concatenate([both, only_b])))
    plan["cancel_rows"] = np.sort(both)
    layers.append(planted_layer(T_ALLNEG, rng.uniform(0.5, 2.0, 300), spread(base, rows, uns[:60:2], 10, start=37)))
    # the filter classes' landmark: a term on the FIRST row of 30 segments (and elsewhere)
    first = np.concatenate([base[uns[5:35]], spread(base, rows, uns[40:50], 5, start=41)])
    layers.append(planted_layer(T_FIRSTROW, np.concatenate([2.5 - 0.01 * np.arange(30), rng.uniform(0.2, 1.0, 50)]), first))
    plan["first_rows"] = base[uns[5:35]]
    # long queries: 64 terms of 400 rows each
    for j in range(64):
        layers.append(planted_layer(T_LONG0 + j, rng.uniform(0.2, 2.2, 400), np.sort(rng.choice(n, 400, replace=False))))
    off, idx, val = assemble(n, layers)
    # folders: 1 = rows of unsampled segments only (a class the sample cannot see), 2 = five rows, 3 = no row (never
    # used), 4 = the first rows of segments
    folder = np.zeros(n, np.int32)
    folder[np.isin(segment_of(np.arange(n), base), uns[:40])] = 1
    folder[plan["invisible_strong"][:5]] = 2
    folder[plan["first_rows"]] = 4
    plan["folder"] = folder
    return off, idx, val, plan


T_EA, T_EB, T_FA, T_FB, T_G, T_C2, T_H1, T_H2, T_I, T_HUGE, T_N = 84, 85, 86, 87, 88, 91, 92, 93, 94, 95, 97
HUGE = 1.0e7


def wave0_rows(base, count):
    """count rows of the segment at `base` that thread t < 64 of a 256-thread block owns, each thread at most one of them:
    the full scan of inv_scan_segments hands them all to wave 0, whose list they fill"""
    b = np.arange(count)
    assert count <= 64
    return base + 256 * (b % 16) + b


def corpus_p():
    """Geometry P: 5 x 4096 rows in one upsert (5 full segments; per-query blocks own one segment each, or, with
    VR_SPARSE_BATCH_BLOCKS=1, one block walks all five). Layers:
      T_BALLAST  every row (df = N: idf 2.4e-5, never essential); T_C2 every second row (idf ln 2)
      T_SURV     three rare terms that mark 1023 / 1024 / 1025 rows of segment 2 (kInvMaxSurvivors +- 1), after 40 strong
                 rows in each of segments 0 and 1 (wave 0's rows: its list is full after the first segment)
      T_EA/T_EB  table overflow: 450 + 450 postings in segment 2 (> 768), winners among T_EB's last rows (passed on
                 unfiltered once the table is full) and among four rows that carry both; a high seed threshold
      T_FA/T_FB  buffer flush: the same shape in segment 1 under a LOW seed threshold: every named row survives, so the
                 wave buffers more than 448 candidates; the ten best rows carry both terms
      T_G        1500 rows of segment 0: the seed wave stops after kSeedRowsPerWave
      T_H1/T_H2  20 rows each: fewer than max(4 k, 64) expected seed rows, every term essential
      T_I        rows of segments 1..3 only: the seed (segments 0 and 4) finds nothing, every share goes to the full scan
      T_N        the non-essential bound decides: 24 seed rows (odd rows: no T_C2) tie at value 5.0, so the seed threshold IS
                 the final k-th score; six rows of segment 2 carry 4.9 and a T_C2 value above 0.9: their essential sum alone
                 stays below the threshold, T_C2 lifts their score above it, they are the six best
      T_HUGE     ONE posting of 1e7 in segment 3: that segment's vmax makes every term essential, its block flags need_full"""
    ups = GEOMETRIES["p4096"]
    n = sum(ups)
    base, rows = segment_table(ups)
    rng = np.random.default_rng(4096)
    c2 = rng.uniform(0.2, 1.0, n // 2)
    lifted = base[2] + 2 * np.flatnonzero(c2[base[2] // 2:base[3] // 2] > 0.9)[:6]
    n_seeds = np.concatenate([base[0] + 2 * np.arange(12) + 301, base[4] + 2 * np.arange(12) + 301])
    layers = [background_layer(n, VOCAB, 6, 18), planted_layer(T_BALLAST, rng.uniform(0.2, 1.0, n), np.arange(n)),
              planted_layer(T_C2, c2, np.arange(0, n, 2)),
              planted_layer(T_N, np.concatenate([np.full(24, 5.0), np.full(6, 4.9)]), np.concatenate([n_seeds, lifted])),
              planted_layer(T_HUGE, [HUGE], [base[3] + 77])]
    plan = {"n": n, "seg_base": base, "seg_rows": rows, "n_seg": base.shape[0], "lifted": lifted}
    for t, m in zip(T_SURV, (kInvMaxSurvivors - 1, kInvMaxSurvivors, kInvMaxSurvivors + 1)):
        head = np.concatenate([wave0_rows(base[0], 40), wave0_rows(base[1], 40)])
        mid = base[2] + np.sort(rng.choice(int(rows[2]), m, replace=False))
        late = spread(base, rows, [3, 4], 20, start=t + 1)
        layers.append(planted_layer(t, np.concatenate([rng.uniform(5.0, 6.0, head.shape[0]), rng.uniform(7.0, 9.5, m),
                                                       rng.uniform(8.0, 9.4, late.shape[0])]), np.concatenate([head, mid, late])))
    i = np.arange(450)
    for (ta, tb), seg, seed_lo, seed_hi, n_both, win_a in (((T_EA, T_EB), 2, 7.0, 8.0, 4, 6.0), ((T_FA, T_FB), 1, 0.5, 1.0, 10, 7.5)):
        off_a, off_b = (1, 4) if seg == 2 else (2, 5)
        b_rows = base[seg] + 9 * i + off_b
        a_rows = np.concatenate([base[seg] + 9 * i[:450 - n_both] + off_a, b_rows[450 - n_both:]])
        b_val = rng.uniform(4.0, 6.0, 450)
        b_val[400:410] = 8.6 + 0.02 * np.arange(10)      # winners that only T_xB names, after the table is full
        b_val[450 - n_both:] = 8.9 + 0.005 * np.arange(n_both)
        a_val = rng.uniform(4.0, 6.0, 450)
        a_val[450 - n_both:] = win_a
        others = [s for s in range(5) if s != seg]
        a_else = spread(base, rows, others, 37, start=11)  # 148 more rows: df 598
        seeds = spread(base, rows, [0, 4], 15, start=21)   # T_xB in the segments the seed reads
        third = spread(base, rows, [3], 10, start=31)      # winners in the segment whose block flags need_full
        rest = spread(base, rows, [s for s in others if s not in (0, 4, 3)], 10, start=33)
        layers.append(planted_layer(ta, np.concatenate([a_val, rng.uniform(4.0, 6.0, a_else.shape[0])]), np.concatenate([a_rows, a_else])))
        layers.append(planted_layer(tb, np.concatenate([b_val, rng.uniform(seed_lo, seed_hi, 30), 8.65 + 0.015 * np.arange(10),
                                                        rng.uniform(4.0, 6.0, rest.shape[0])]), np.concatenate([b_rows, seeds, third, rest])))
    g_rows = np.concatenate([base[0] + 2 * np.arange(1500) + 1, spread(base, rows, [1, 2, 3, 4], 25, start=43)])
    g_val = rng.uniform(0.5, 2.0, g_rows.shape[0])
    g_val[1400:1410] = 3.0 + 0.01 * np.arange(10)          # winners the seed never reaches
    g_val[1500::10] = 2.9
    layers.append(planted_layer(T_G, g_val, g_rows))
    layers.append(planted_layer(T_H1, rng.uniform(0.5, 2.0, 20), spread(base, rows, range(5), 4, start=51)))
    layers.append(planted_layer(T_H2, rng.uniform(0.5, 2.0, 20), spread(base, rows, range(5), 4, start=53)))
    layers.append(planted_layer(T_I, rng.uniform(0.5, 2.0, 30), spread(base, rows, [1, 2, 3], 10, start=57)))
    off, idx, val = assemble(n, layers)
    return off, idx, val, plan


def p_queries():
    """name -> (ids, values, k) of the geometry P cases (IDF weights: the engine's own statistics)"""
    q = lambda ids, vals=None: (np.array(ids, np.int32), np.ones(len(ids), np.float32) if vals is None else np.array(vals, np.float32))
    return {
        "table": q([T_C2, T_EA, T_EB]), "flush": q([T_BALLAST, T_FA, T_FB]), "seed_stops": q([T_BALLAST, T_G]),
        "all_essential": q([T_H1, T_H2]), "no_seed": q([T_I]), "ne_bound": q([T_C2, T_N]),
    }


def term_postings(off, idx, val, term):
    """(rows ascending, values) of one term: its postings"""
    at = np.flatnonzero(idx == term)
    return np.searchsorted(off, at, side="right") - 1, val[at]


def segment_vmax(off, idx, val, seg_base):
    """the largest |value| among the postings of every segment (InvSeg::pad)"""
    row_of = np.repeat(np.arange(off.shape[0] - 1), np.diff(off))
    return np.maximum.reduceat(np.abs(val), np.searchsorted(row_of, seg_base))


def seed_segments(n_seg, gs):
    """{(block, wave): [segments]} of the seed pass: unit u = segment kSeedStride * u; block bx takes units bx, bx + gs,
    ..., its wave w every kInvWaves-th of them"""
    n_units = -(-n_seg // kSeedStride)
    out = {}
    for bx in range(gs):
        units = list(range(bx, n_units, gs))
        for w in range(kInvWaves):
            if units[w::kInvWaves]:
                out[(bx, w)] = [u * kSeedStride for u in units[w::kInvWaves]]
    return out


def seed_rows(off, idx, val, seg_base, seg_rows, essential_terms, segments):
    """The rows ONE wave of the seed pass scores: it walks `segments` in order and, per segment, the essential terms' runs
    (in t_ord order) 64 postings at a time, until it has kSeedRowsPerWave rows; a term that starts after that still gets
    one round. -> (rows in the order scored, rows the terms name in these segments)"""
    got, named = [], 0
    for s in segments:
        runs = []
        for t in essential_terms:
            r, _ = term_postings(off, idx, val, t)
            runs.append(r[(r >= seg_base[s]) & (r < seg_base[s] + seg_rows[s])])
        named += sum(len(r) for r in runs)
        if len(got) >= kSeedRowsPerWave:
            continue
        for r in runs:
            for p in range(0, len(r) + 1, 64):
                got += r[p:p + 64].tolist()
                if len(r[p:p + 64]) < 64 or len(got) >= kSeedRowsPerWave:
                    break
    return np.array(got, np.int64), named


def seed_threshold(scores, passing, rows, k):
    """the seed's k-th score among the rows it scored (None: fewer than k of them pass and share a term)"""
    sc = np.asarray(scores, np.float32)[np.unique(rows)] if len(rows) else np.zeros(0, np.float32)
    if passing is not None and len(rows):
        sc = sc[np.asarray(passing, bool)[np.unique(rows)]]
    sc = np.sort(sc[sc > -np.inf])[::-1]
    return float(sc[k - 1]) if sc.shape[0] >= k else None


def per_query_model(csr, plan, oracle, q_idx, q_val, k, nq, env_blocks=None, passing=None):
    """The per-query route (kSeedPruned) for one query of a batch of nq: the seed's essential terms, the rows it scores and
    its threshold, then per block of the main pass whether it prunes. -> dict with seed_ne, seed_margin, seed_scored,
    seed_named, theta, blocks = [(segments, vmax, n_ne, prunes, margin)], margin = the smallest margin relied on."""
    off, idx, val = csr
    ids, w, frac = query_weights(oracle, q_idx, q_val)
    order, _ = term_order(w)
    gx, gs = blocks_per_query(nq, plan["n_seg"], env_blocks)
    ne, m_seed = seed_essential(w, frac, oracle.n_points, k)
    scored, named = [], 0
    if ne is not None:
        for segs in seed_segments(plan["n_seg"], gs).values():
            r, n = seed_rows(off, idx, val, plan["seg_base"], plan["seg_rows"], ids[order[ne:]], segs)
            scored.append(r)
            named += n
    scored = np.concatenate(scored) if scored else np.zeros(0, np.int64)
    theta = seed_threshold(oracle.scores(q_idx, q_val), passing, scored, k)
    vmax = segment_vmax(off, idx, val, plan["seg_base"])
    blocks = []
    for bx in range(gx):
        segs = share_of_block(plan["n_seg"], gx, bx)
        vm = float(vmax[segs].max())
        blocks.append((segs, vm) + block_prunes(w, frac, theta, vm))
    return {"ids": ids, "w": w, "frac": frac, "order": order, "seed_ne": ne, "seed_margin": m_seed, "seed_scored": scored.shape[0],
            "seed_named": named, "theta": theta, "blocks": blocks, "margin": min([m_seed] + [b[4] for b in blocks])}


def pruned_wave_walk(runs):
    """sparse_inv_pruned_kernel<false>, one wave, one segment: runs = the essential terms' posting counts in the segment,
    in walk order (ascending |weight|). Postings are taken 64 at a time; a round that starts with h_used >= 768 passes its
    rows on unfiltered. -> (postings that went through the table, postings passed on, per run the first posting passed on
    or None)."""
    h_used, tabled, direct, first = 0, 0, 0, []
    for n in runs:
        f = None
        for p in range(0, max(n, 1), 64):
            c = min(64, n - p)
            if h_used >= PRUNED_TABLE_ROWS:
                direct += c
                f = p if f is None else f
            else:
                tabled += c
            h_used += c
        first.append(f)
    return tabled, direct, first


# ---- geometry R: segments of chosen posting counts for the 64-way searches ---------------------------------------------

R_UPSERTS = [1, 64, 65, 4096, 4096, 4096]
R_LIGHT = (100, 200, 300)                     # the terms of the light segments (one posting per row)
R_COMMON0, R_COMMON_STEP = 1000, 10           # 64 terms every row of the deep segment carries
R_RUNS = ((900, 1), (1005, 64), (1015, 65), (1025, 256), (1035, 257), (2000, 512))  # (term, run length) in the deep segment
R_ABSENT = (50, 150, 950, 1001, 1999, 2500)   # ids below, between and above the segments' terms


def corpus_r():
    """Segments of 1, 64, 65, 4096, more than 64^3 (4096 rows x 64 terms + runs of 1, 64, 65, 256, 257 and 512) and 4097
    postings. In the deep segment 900 is the smallest id (a run of one, the first posting) and 2000 the largest: its run of
    512 ends exactly at the segment's last posting. The deep segment is segment 4: the seed pass (every fourth) walks it."""
    n = sum(R_UPSERTS)
    base, rows = segment_table(R_UPSERTS)
    rng = np.random.default_rng(64)
    r = np.arange(n)
    light = np.flatnonzero((r < base[4]) | (r >= base[5]))
    layers = [planted_layer(0, rng.uniform(0.2, 2.2, light.shape[0]), light)]
    layers[0] = (light, np.array(R_LIGHT, np.int32)[light % 3], layers[0][2])
    layers.append(planted_layer(R_LIGHT[1], [1.5], [base[5] + 3 + (0 if (base[5] + 3) % 3 != 1 else 1)]))  # the 4097th posting
    deep = np.arange(base[4], base[4] + rows[4])
    for j in range(64):
        layers.append(planted_layer(R_COMMON0 + R_COMMON_STEP * j, rng.uniform(0.2, 2.2, deep.shape[0]), deep))
    for t, m in R_RUNS:
        layers.append(planted_layer(t, rng.uniform(0.2, 2.2, m), base[4] + np.sort(rng.choice(int(rows[4]), m, replace=False))))
    off, idx, val = assemble(n, layers)
    return off, idx, val, {"n": n, "seg_base": base, "seg_rows": rows, "n_seg": base.shape[0]}


def r_terms():
    return list(R_LIGHT) + [R_COMMON0, R_COMMON0 + 63 * R_COMMON_STEP] + [t for t, _ in R_RUNS] + list(R_ABSENT)


FOLDER_TIE_OUT = 5  # the folder of ONE member of the tie group: SearchFilter(exclude_folders=[5]) filters it out


def live_rows(off, idx, plan):
    """(live, dead, folder) of a geometry-S engine: two members of the tie group and 40 rows that carry no planted term are
    deleted (a planted df stays as chosen), a third member of the tie group moves to FOLDER_TIE_OUT"""
    n = plan["n"]
    row_of = np.repeat(np.arange(n), np.diff(off))
    planted = np.zeros(n, bool)
    planted[row_of[idx < BACKGROUND_TERM0]] = True
    tie = plan["tie_rows"]
    dead = np.concatenate([tie[[3, 40]], np.random.default_rng(n).choice(np.flatnonzero(~planted), 40, replace=False)])
    live = np.ones(n, bool)
    live[dead] = False
    folder = plan["folder"].copy()
    folder[tie[10]] = FOLDER_TIE_OUT
    return live, dead, folder


def planted_queries():
    """name -> (ids, values) of the planted S queries (one term unless said otherwise)"""
    one = lambda t: (np.array([t], np.int32), np.ones(1, np.float32))
    long_ids = (T_LONG0 + np.arange(64)).astype(np.int32)
    lw = np.random.default_rng(3).uniform(0.5, 1.5, 64).astype(np.float32)
    return {
        "invisible": one(T_INVISIBLE), "only64": one(T_ONLY64), "only65": one(T_ONLY65), "flood": one(T_FLOOD),
        "tail": one(T_TAIL), "last": one(T_LAST), "neartail": one(T_NEAR), "tie": one(T_TIE),
        # a negative k-th score: rows with T_POS above rows with only T_NEG
        "mixed": (np.array([T_POS, T_NEG], np.int32), np.array([1.0, -1.0], np.float32)),
        # products that cancel to exactly +0.0 (equal dfs: equal idf), above the negative rows
        "cancel": (np.array([T_CANCEL_A, T_CANCEL_B], np.int32), np.array([-1.0, 1.0], np.float32)),
        "allneg": (np.array([T_ALLNEG], np.int32), np.array([-1.0], np.float32)),
        "long24": (long_ids[:24], lw[:24]), "long32": (long_ids[:32], lw[:32]), "long33": (long_ids[:33], lw[:33]),
        "long28b": (long_ids[36:64], -lw[36:64]),
        # 32 terms disjoint from long32's: the two share a group whose union is exactly kGrpMaxU = 64 (one run per lane)
        "long32c": (long_ids[32:64], lw[32:64]),
        "absent": one(T_ABSENT), "none": (np.zeros(0, np.int32), np.zeros(0, np.float32)),
        "repeat": (np.array([T_TAIL, T_LAST, T_TAIL], np.int32), np.array([1.0, 0.5, 7.0], np.float32)),
    }


PLANTED_ORDER = ("invisible", "only64", "only65", "tail", "last", "neartail", "tie", "mixed", "cancel", "allneg", "long24", "long32",
                 "long33", "long32c", "long28b", "absent", "none", "repeat")


def planted_batch(nq, shift=0, flood=False):
    """(queries, {name: position}): the planted queries among riders. Positions 3 j + shift + (j % 2) are all even for
    shift = 0 and all odd for shift = 1 (with groups of two: first or second of a pair); "invisible" is followed by a partner with the same term (it shares
    its block), the others sit among riders that share nothing with them. flood: "flood" takes the last position."""
    pq = planted_queries()
    assert nq < 40 or nq >= 3 * len(PLANTED_ORDER) + 3
    names = list(PLANTED_ORDER) if nq >= 40 else ["invisible", "only65", "tie", "mixed", "long33", "neartail"]
    at = {}
    for j, name in enumerate(names):
        at[name] = (3 * j + shift + (j % 2)) % nq
    qs = riders(nq, VOCAB, 1000 + nq + shift)
    for name, i in at.items():
        qs[i] = pq[name]
    if "invisible" in at and shift == 0:
        qs[at["invisible"] + 1] = (np.array([T_INVISIBLE, BACKGROUND_TERM0 + 50 * BACKGROUND_STEP], np.int32), np.array([1.0, 0.3], np.float32))
    if flood:
        at["flood"] = nq - 1
        qs[nq - 1] = pq["flood"]
    assert len(set(at.values())) == len(at)
    if nq >= 40:
        # long24, long32, long32c, long28b are neighbours in the host's order (inv_group_queries): whether long32 pairs with
        # long24 (union 32) or with long32c (union exactly kGrpMaxU = 64: one run per lane, none to spare) depends on the
        # parity of the queries before them; a rider that leaves the batch (no terms) flips it
        if max(u for _, u in group_queries(qs)) < kGrpMaxU:
            free = [i for i in range(nq) if i not in at.values() and i != at["invisible"] + 1]
            qs[free[-1]] = pq["none"]
        assert ([at["long32"], at["long32c"]], kGrpMaxU) in group_queries(qs)
    return qs, at
