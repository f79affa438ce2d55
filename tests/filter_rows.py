"""TEST INFRASTRUCTURE shared by test_filter_rows_cpu.py and test_filter_rows_gpu.py: corpora whose payload columns make
every probed row's PASS BIT the answer of a search, on every route that consumes a filter (voitta_rag_amd/csrc/filter.hip:
filter_mask_kernel's bytes, filter_planes_kernel's bit planes). NumPy only; no device, no scores.

Corpus. n rows x DIM, seeded; row i carries a sparse vector with one term of its own (UNIQUE0 + i), one term every row
carries (COMMON) and three of a small background vocabulary. Two sizes: N_SMALL (the exact scan) and N_BIG (above the
thresholds of the two-stage and of the batched scan, with n % 32 = 5, n % 64 = n % 256 = 37), stored in several upserts
(UPSERTS) so that the engine's capacity grows.

Payload columns. Neighbours differ: the folder id follows i % 7, the index-folder id i % 5, `modified` i % 13 and
`created` i % 11, and none of 1, 32, 64, 256 is a multiple of any of these primes; the folder classes alone (1 .. 4, 15, 16,
20) tell any two folder ids apart, so rows i, i +- 1, i +- 32, i +- 64 and i +- 256 never share their whole pass pattern.
Folder ids are sparse (FOLDER_TABLE: 0 .. MAX_FOLDER = 3999, so a folder pass table has 4,000 entries and an index-folder
table 41: the concatenated tables of a batch's classes differ in length and offset). Planted on top: the timestamp-edge
rows (edge_rows: each of LO - 1, LO, HI, HI + 1, 0, a negative value, INT64_MIN + 1, INT64_MAX and absent on either
column, the other column in range; absent next to an in-range column is therefore among them), ONE row of folder ONE_FOLDER, and folder LAST_FOLDER on every second row of the last partial
32-row plane word, the last row among them. Tombstones (dead_rows) are a spread of the probes, deleted after the upsert.

Classes. CLASSES: about 20 filters as plain Spec records (the fields of voitta_rag_amd.SearchFilter; filters() builds the
real ones). class_mask() restates oracle_mask of test_batch_filters_gpu.py, term for term. `kind` says what a class is
defined as: "all" (no condition: every live row passes), "none" (no row can pass: an exclude set naming every id, an empty
intersection, lo > hi) or "mixed" (some probes pass, some fail: test_filter_rows_cpu.py holds every class to its kind).

Probes. probe_rows(): rows 0 .. 130, each side of the first and last multiples of 256, of 4,096 and of 16,384, the last 70
rows, the edge rows, the folder-edge rows, the tombstones.

Expected answers, from the masks alone:
  dense   the query of probe r is row r's own vector: under class c, r is returned, and first, iff mask_c[r]; every
          returned row satisfies mask_c. (Cosine of a row with itself is the largest score there is; the rows are
          pairwise distinct Gaussian vectors.)
  sparse  the query of probe r is (UNIQUE0 + r, COMMON): the term only r carries outweighs the common one (idf of a term
          of one row against idf of a term of all rows: ln(N) against 1 / (2 N)), so the same two statements hold; every row
          carries COMMON, so every passing row is a hit.
check_probe() asserts both statements for one answer.

Mutants. mutants() lists wrong predicates as functions of the corpus; test_filter_rows_cpu.py proves that each changes the
pass bit of at least one probe under at least one class, at both sizes: the GPU tests would notice any of them.

Every number below that restates a constant of voitta_rag_amd/csrc is read back from the sources by
test_filter_rows_cpu.py: kPlaneClasses (filter.hip), the row thresholds PREFILTER_MIN_ROWS (prefilter.hip) and
BATCH_MIN_ROWS (batch.hip), kQueryBlock, kFusedMaxK, kMaxK and kInvMaxTerms (engine_internal.h)."""
from dataclasses import asdict, dataclass, field

import numpy as np

ABSENT = -(2**63)
INT64_MIN1, INT64_MAX = -(2**63) + 1, 2**63 - 1
DIM = 128
N_SMALL, N_BIG = 1_300, 16_421
UPSERTS = {N_SMALL: (700, 13, 587), N_BIG: (7000, 13, 9000, 408)}

kPlaneClasses = 8          # filter.hip: classes per grid.y step of filter_planes_kernel
kQueryBlock = 16           # engine_internal.h: the batched scan takes more than this many queries
kFusedMaxK = 64            # engine_internal.h: ... of k <= 64
kMaxK = 1024               # engine_internal.h: largest k of a search
kInvMaxTerms = 32          # engine_internal.h: distinct terms the inverted scans take
PREFILTER_MIN_ROWS = 4096  # prefilter.hip: the two-stage scan
BATCH_MIN_ROWS = 16384     # batch.hip: the batched scan
GROUPED_MIN_QUERIES = 16   # invert.hip, inv_grouped_fits: the grouped sparse scan

FOLDER_TABLE = np.array([0, 5, 64, 256, 1023, 2048, 3999], np.int32)
MAX_FOLDER = 3999
ONE_FOLDER, LAST_FOLDER = 2500, 3000   # one row; rows of the last partial plane word only
ONE_ROW = 95                           # the last row of plane word 2
IFOLDER_TABLE = np.array([0, 1, 2, 3, 40], np.int32)
LO, HI = 1000, 2000
NEGATIVE = -5
EDGE_VALUES = (LO - 1, LO, HI, HI + 1, 0, NEGATIVE, INT64_MIN1, INT64_MAX, ABSENT)
EDGE_ROW0, EDGE_STEP = 140, 3          # edge row j sits at EDGE_ROW0 + EDGE_STEP * j (beyond the probes 0 .. 130)
IN_RANGE = 1500

COMMON, BACKGROUND0, BACKGROUND_VOCAB, UNIQUE0 = 1, 10, 50, 1000


# ---- corpus ---------------------------------------------------------------------------------------------------------

def edge_rows():
    """[(row, column, value)]: `column` of `row` holds `value`, the other column IN_RANGE"""
    out = []
    for c, col in enumerate(("modified", "created")):
        for j, v in enumerate(EDGE_VALUES):
            out.append((EDGE_ROW0 + EDGE_STEP * (c * len(EDGE_VALUES) + j), col, v))
    return out


def last_word_rows(n):
    """the rows of the last partial 32-row word that carry LAST_FOLDER: every second one, counted from the last row"""
    first = n // 32 * 32
    assert first < n, "n is a multiple of 32: no partial word"
    return np.arange(n - 1, first - 1, -2)[::-1]


def corpus(n, seed=None):
    """dict of the host copy: x (n x DIM f32), sparse CSR (off, idx, val), folder, ifolder, created, modified; no row is
    dead yet (live all True): delete(h, rows) keeps the copy in step with Engine.delete_rows."""
    rng = np.random.default_rng(n if seed is None else seed)
    i = np.arange(n)
    x = rng.standard_normal((n, DIM)).astype(np.float32)
    folder = FOLDER_TABLE[i % 7].copy()
    ifolder = IFOLDER_TABLE[i % 5].copy()
    modified = (400 + 150 * (i % 13)).astype(np.int64)   # 400 .. 2200: below, inside and above [LO, HI]
    created = (500 + 200 * (i % 11)).astype(np.int64)    # 500 .. 2500
    modified[i % 17 == 3] = ABSENT
    created[i % 19 == 5] = ABSENT
    for row, col, v in edge_rows():
        (modified if col == "modified" else created)[row] = v
        (created if col == "modified" else modified)[row] = IN_RANGE
    folder[ONE_ROW] = ONE_FOLDER
    folder[last_word_rows(n)] = LAST_FOLDER
    # sparse: COMMON, three distinct background terms, the row's own term; ascending ids
    bg = BACKGROUND0 + np.sort(np.stack([(3 * i + 17 * j) % BACKGROUND_VOCAB for j in range(3)], axis=1), axis=1)
    idx = np.concatenate([np.full((n, 1), COMMON), bg, (UNIQUE0 + i)[:, None]], axis=1).astype(np.int32)
    assert np.all(np.diff(idx, axis=1) > 0)
    val = rng.uniform(0.2, 2.2, size=idx.shape).astype(np.float32)
    off = (np.arange(n + 1) * idx.shape[1]).astype(np.int64)
    return dict(n=n, x=x, off=off, idx=idx.reshape(-1), val=val.reshape(-1), folder=folder, ifolder=ifolder, created=created,
                modified=modified, live=np.ones(n, bool))


def upsert_all(e, h, upserts=None, first=0):
    """store rows first .. n of the host copy in the given upsert sizes"""
    at = first
    for m in upserts or UPSERTS[h["n"]]:
        a, b = h["off"][at], h["off"][at + m]
        e.upsert(h["x"][at:at + m], sparse=(h["off"][at:at + m + 1] - a, h["idx"][a:b], h["val"][a:b]),
                 folder_ids=h["folder"][at:at + m], index_folder_ids=h["ifolder"][at:at + m], created=h["created"][at:at + m],
                 modified=h["modified"][at:at + m])
        at += m
    assert at == h["n"]


def delete(h, rows):
    h["live"][np.asarray(rows, np.int64)] = False


def take_rows(h, keep):
    """the host copy of the rows `keep` (ascending), renumbered in order: what compact() leaves"""
    keep = np.asarray(keep, np.int64)
    w = int(h["off"][1] - h["off"][0])
    pick = (keep[:, None] * w + np.arange(w)[None, :]).reshape(-1)
    out = {c: h[c][keep].copy() for c in ("x", "folder", "ifolder", "created", "modified", "live")}
    out.update(n=keep.shape[0], off=(np.arange(keep.shape[0] + 1) * w).astype(np.int64), idx=h["idx"][pick].copy(),
               val=h["val"][pick].copy())
    return out


def append_rows(h, g):
    """the host copy h followed by the rows of g"""
    out = {c: np.concatenate([h[c], g[c]]) for c in ("x", "folder", "ifolder", "created", "modified", "live", "idx", "val")}
    out.update(n=h["n"] + g["n"], off=np.concatenate([h["off"], h["off"][-1] + g["off"][1:]]))
    return out


# ---- classes --------------------------------------------------------------------------------------------------------

@dataclass
class Spec:
    """the fields of voitta_rag_amd.SearchFilter, and what the class is defined as"""
    kind: str = "mixed"
    folder_filter: int | None = None
    include_folders: list | None = None
    exclude_folders: list = field(default_factory=list)
    exclude_index_folders: list = field(default_factory=list)
    date_start: int | None = None
    date_end: int | None = None
    date_field: str | None = None

    def is_empty(self):
        return (self.folder_filter is None and self.include_folders is None and not self.exclude_folders
                and not self.exclude_index_folders and self.date_start is None and self.date_end is None)


EVERY_FOLDER = sorted(set(FOLDER_TABLE.tolist()) | {ONE_FOLDER, LAST_FOLDER})

# The position in this list is the class's plane when a batch names the classes in this order: 0 .. 7 share the first
# grid.y step of filter_planes_kernel, 8 .. 15 the second, 16 .. the third. None comes first and the empty filter last
# (the engine gives both the same class), so the first m entries are m distinct classes for every m < len(CLASSES).
CLASSES = [
    None,                                                                            # 0  no filter
    Spec(folder_filter=MAX_FOLDER),                                                  # 1  the largest id
    Spec(folder_filter=0),                                                           # 2  id 0
    Spec(include_folders=[5, 256, MAX_FOLDER + 1, 70_000, -3]),                       # 3  ids beyond the largest, a negative id
    Spec(folder_filter=1023, include_folders=[0, 256, 1023, MAX_FOLDER]),            # 4  include and folder_filter: id 1023
    Spec(kind="none", folder_filter=1023, include_folders=[0, 256]),                 # 5  ... an empty intersection
    Spec(kind="none", exclude_folders=EVERY_FOLDER),                                 # 6  an exclude set covering every id
    Spec(exclude_index_folders=[1, 40]),                                             # 7  index folders: the largest id and another
    Spec(date_start=LO),                                                             # 8  lo only (default field: modified)
    Spec(date_end=HI),                                                               # 9  hi only
    Spec(date_start=LO, date_end=HI),                                                # 10 both
    Spec(kind="none", date_start=HI, date_end=LO),                                   # 11 lo > hi
    Spec(date_start=LO, date_end=HI, date_field="created"),                          # 12 the other column
    Spec(date_start=LO, date_field="created"),                                       # 13 ... one-sided
    Spec(date_start=LO, date_end=HI, include_folders=[0, 64, 1023, MAX_FOLDER], exclude_index_folders=[2]),  # 14 range and folders
    Spec(folder_filter=ONE_FOLDER),                                                  # 15 exactly one row
    Spec(folder_filter=LAST_FOLDER),                                                 # 16 rows of the last partial plane word only
    Spec(exclude_folders=[0, 256, MAX_FOLDER], date_end=HI, date_field="created"),   # 17 exclude and hi on created
    Spec(date_start=0, date_field="modified"),                                       # 18 lo = 0, the field named
    Spec(date_end=INT64_MAX, date_field="created"),                                  # 19 hi = INT64_MAX: only absent fails
    Spec(exclude_folders=[64, 256]),                                                 # 20 an exclude set alone
    Spec(kind="all"),                                                                # 21 the empty filter
]
CLASS_COUNTS = (1, 7, 8, 9, 16, 17, len(CLASSES))


def kind_of(spec):
    return "all" if spec is None else spec.kind


def filters(specs=None):
    """the SearchFilter objects of the classes (None stays None)"""
    from voitta_rag_amd import SearchFilter

    out = []
    for s in CLASSES if specs is None else specs:
        if s is None:
            out.append(None)
        else:
            kw = asdict(s)
            kw.pop("kind")
            out.append(SearchFilter(**kw))
    return out


def class_mask(f, h):
    """oracle_mask of test_batch_filters_gpu.py, restated: the rows of host copy h that pass filter (or Spec) f"""
    m = h["live"].copy()
    if f is None or f.is_empty():
        return m
    if f.folder_filter is not None:
        m &= h["folder"] == f.folder_filter
    if f.include_folders is not None:
        m &= np.isin(h["folder"], f.include_folders)
    if f.exclude_folders:
        m &= ~np.isin(h["folder"], f.exclude_folders)
    if f.exclude_index_folders:
        m &= ~np.isin(h["ifolder"], f.exclude_index_folders)
    if f.date_start is not None or f.date_end is not None:
        ts = h["created"] if f.date_field == "created" else h["modified"]
        m &= ts != ABSENT
        if f.date_start is not None:
            m &= ts >= f.date_start
        if f.date_end is not None:
            m &= ts <= f.date_end
    return m


def masks(h, specs=None):
    """(n_classes, n) bool"""
    return np.stack([class_mask(s, h) for s in (CLASSES if specs is None else specs)])


# ---- probes ---------------------------------------------------------------------------------------------------------

def probe_rows(n):
    """ascending distinct rows"""
    p = set(range(0, 131))
    top = n // 256
    for m in sorted({1, 2, 3, 4, top - 2, top - 1, top}):
        if m >= 1:
            p |= {256 * m - 1, 256 * m, 256 * m + 1}
    for edge in (PREFILTER_MIN_ROWS, BATCH_MIN_ROWS):
        p |= {edge - 2, edge - 1, edge, edge + 1}
    p |= set(range(n - 70, n))
    p |= {r for r, _, _ in edge_rows()}
    p |= {ONE_ROW, ONE_ROW + 1} | set(last_word_rows(n).tolist())
    p |= {r for r in range(200, 260) if FOLDER_TABLE[r % 7] in (0, MAX_FOLDER)}  # (more rows of the ids 0 and 3999)
    return np.array(sorted(r for r in p if 0 <= r < n), np.int64)


def dead_rows(n):
    """The tombstones: every seventh probe (never an edge row, the one row of ONE_FOLDER or a LAST_FOLDER row), and a
    spread of other rows."""
    keep = {r for r, _, _ in edge_rows()} | {ONE_ROW} | set(last_word_rows(n).tolist())
    p = [int(r) for r in probe_rows(n)[3::7] if int(r) not in keep]
    other = [r for r in range(133, n, 97) if r not in keep]
    return np.array(sorted(set(p) | set(other)), np.int64)


def more_dead_rows(n):
    """further probes to delete later (the state-change test): every seventh from the fifth on, with the same exceptions"""
    keep = {r for r, _, _ in edge_rows()} | {ONE_ROW} | set(last_word_rows(n).tolist())
    return np.array([int(r) for r in probe_rows(n)[5::7] if int(r) not in keep], np.int64)


def dense_query(h, r):
    return h["x"][r]


def sparse_query(r, pad=0):
    """(ids, values): the term only row r carries, then COMMON; pad: that many more terms no row carries (more than
    kInvMaxTerms distinct terms in all: the forward scan)"""
    ids = [UNIQUE0 + int(r), COMMON] + [2_000_000 + j for j in range(pad)]
    return np.array(ids, np.int32), np.ones(len(ids), np.float32)


def check_probe(rows, r, mask, tag):
    """the two statements about one answer: r is returned, and first, iff it passes; every returned row passes"""
    rows = np.asarray(rows)
    assert mask[rows].all(), (tag, "a returned row fails the filter", rows[~mask[rows]][:8].tolist())
    if mask[r]:
        assert rows.shape[0] > 0 and rows[0] == r, (tag, "the probe passes and is not first", rows[:4].tolist())
    else:
        assert r not in rows.tolist(), (tag, "the probe fails and is returned")


def sample_pairs(n_probes, n_classes, count=240, seed=7):
    """`count` distinct (probe index, class index) pairs, seeded: the answers compared in full against oracle.core"""
    rng = np.random.default_rng(seed)
    flat = rng.choice(n_probes * n_classes, size=min(count, n_probes * n_classes), replace=False)
    return [(int(f) // n_classes, int(f) % n_classes) for f in np.sort(flat)]


# ---- mutants: wrong predicates the probes have to tell from the right one ---------------------------------------------

def _shift(m, s):
    out = np.zeros_like(m)
    out[:, s:] = m[:, :-s]   # row i answers with row i - s's bit
    return out


def _reverse_words(m):
    n = m.shape[1]
    pad = np.zeros((m.shape[0], -(-n // 32) * 32), bool)
    pad[:, :n] = m
    return pad.reshape(m.shape[0], -1, 32)[:, :, ::-1].reshape(m.shape[0], -1)[:, :n]


def _tail(m, value):
    out = m.copy()
    out[:, m.shape[1] // 64 * 64:] = value
    return out


def _date_mutant(h, ge=np.greater_equal, le=np.less_equal, absent_passes=False, swap=False):
    out = []
    for s in CLASSES:
        if s is None or (s.date_start is None and s.date_end is None):
            out.append(class_mask(s, h))
            continue
        bare = Spec(**{**asdict(s), "date_start": None, "date_end": None})
        m = class_mask(bare, h)
        created = (s.date_field == "created") != swap
        ts = h["created"] if created else h["modified"]
        one_sided = (s.date_start is None) != (s.date_end is None)
        if not (absent_passes and one_sided):
            m &= ts != ABSENT
        if s.date_start is not None:
            m &= ge(ts, s.date_start)
        if s.date_end is not None:
            m &= le(ts, s.date_end)
        out.append(m)
    return np.stack(out)


def _next_folder_table(h):
    """class c keeps its date range and takes the folder and index-folder conditions of class c + 1 (the last: of class 0)"""
    out = []
    for c, s in enumerate(CLASSES):
        nxt = CLASSES[(c + 1) % len(CLASSES)]
        base = asdict(nxt) if nxt is not None else asdict(Spec())
        own = asdict(s) if s is not None else asdict(Spec())
        for key in ("date_start", "date_end", "date_field"):
            base[key] = own[key]
        out.append(class_mask(Spec(**base), h))
    return np.stack(out)


def mutants(h):
    """name -> (n_classes, n) bool: what a subtly wrong predicate would answer on host copy h"""
    m = masks(h)
    every = dict(h, live=np.ones(h["n"], bool))
    return {
        "shifted by 1 row": _shift(m, 1), "shifted by 32 rows": _shift(m, 32), "shifted by 64 rows": _shift(m, 64),
        "bit order reversed inside a 32-row word": _reverse_words(m),
        "rows past the last full 64-row group fail": _tail(m, False),
        "rows past the last full 64-row group pass": _tail(m, True),
        "> for >= at lo": _date_mutant(h, ge=np.greater), "< for <= at hi": _date_mutant(h, le=np.less),
        "absent passes a one-sided range": _date_mutant(h, absent_passes=True),
        "created and modified swapped": _date_mutant(h, swap=True),
        "the next class's folder table": _next_folder_table(h),
        "classes of index >= 8 evaluated as class index - 8":
            np.stack([m[c - kPlaneClasses if c >= kPlaneClasses else c] for c in range(len(CLASSES))]),
        "tombstones ignored": masks(every),
    }
