"""What the search entry points launch, for comparing two builds of the library (profiles/search_split_checks.md).

Without arguments: builds the build_small() corpus of tests/test_batch_filters_gpu.py and makes one call each of
search_dense (1, 16 and 300 queries), search_sparse, search_hybrid, search_sparse_batch, search_hybrid_batch,
search_dense_multi and search_hybrid_batch_multi. Run it under `rocprofv3 --kernel-trace --output-format csv -d DIR --`.

--compare DIR_A DIR_B: reads the *kernel_trace.csv of two such runs (one per process of a run) and checks that the launch count, the multiset of
(kernel, grid, workgroup) and, per queue / stream (numbered by first appearance), the order of launches are equal.
Exit status 1 when they are not."""
import collections
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np

    import test_batch_filters_gpu as t

    e, h = t.build_small()
    q, sq, limits, weights, flt = t.make_batch(h, nq=300, seed=5)
    for nq in (1, 16, 300):
        e.search_dense(q[:nq], 10)
    ids, vals = next(s for s in sq if 0 < len(s[0]) <= 32)
    e.search_sparse(ids, vals, 10)
    e.search_hybrid(q[0], ids, vals, 10, 0.1)
    e.search_sparse_batch(sq, 10)
    e.search_hybrid_batch(q, sq, 10, 0.1)
    e.search_dense_multi(q, 10, flt)
    e.search_hybrid_batch_multi(q, sq, limits, weights, flt)
    print(np.asarray(sorted(e.stats().items()), dtype=object).tolist())
    e.close()


def launches(d):
    """The launches of a run as (stream, kernel, (grid, workgroup)) in dispatch order. A run that started child processes
    left one trace per process: their streams are told apart, and compare() matches streams by what they launched."""
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert files, d
    seen, out, lane = {}, [], None
    for path in files:
        with open(path, newline="") as f:
            rows = list(csv.DictReader(f))
        if not rows:  # (a process that launched nothing)
            continue
        order = "Dispatch_Id" if "Dispatch_Id" in rows[0] else "Start_Timestamp"
        rows.sort(key=lambda r: int(r[order]))
        lane = next((c for c in ("Stream_Id", "Queue_Id") if c in rows[0]), None)
        for r in rows:
            shape = tuple(int(r[f"{a}_Size_{x}"]) for a in ("Grid", "Workgroup") for x in "XYZ")
            s = seen.setdefault((path, r[lane] if lane else 0), len(seen))
            out.append((s, r["Kernel_Name"], shape))
    return out, lane


def compare(a, b):
    la, lane = launches(a)
    lb, _ = launches(b)
    print(f"launches: {len(la)} and {len(lb)}; streams told apart by {lane}")
    ca, cb = (collections.Counter((n, s) for _, n, s in x) for x in (la, lb))
    ok = len(la) == len(lb) and ca == cb
    for key in sorted(set(ca) | set(cb)):
        if ca[key] != cb[key]:
            print(f"  {ca[key]:6d} {cb[key]:6d}  {key[0][:90]} {key[1]}")
    print(f"multiset of (kernel, grid, workgroup): {'equal' if ca == cb else 'DIFFERENT'} ({len(ca)} distinct)")
    per = [collections.defaultdict(list), collections.defaultdict(list)]
    for p, x in zip(per, (la, lb)):
        for s, n, shape in x:
            p[s].append((n, shape))
    # streams are numbered by first appearance, which can differ when two streams start at once: match them by content
    same_order = sorted(map(tuple, per[0].values())) == sorted(map(tuple, per[1].values()))
    print(f"per-stream order: {'equal' if same_order else 'DIFFERENT'} ({len(per[0])} and {len(per[1])} streams: "
          f"{sorted(len(v) for v in per[0].values())} launches)")
    return ok and same_order


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(0 if compare(sys.argv[2], sys.argv[3]) else 1)
    run()
