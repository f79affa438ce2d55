"""What the encoder's forward routines launch and return, for comparing two builds of the library
(profiles/encoder_steps_checks.md). VOITTA_ENGINE_LIB selects the library.

python scripts/encoder_launch_sequence.py OUT.npz
    Runs the body below four ways, each in a fresh child process (VR_ENCODE_FUSE and VR_CLS_COLLAPSE are read when a model
    loads): VR_ENCODE_FUSE=1 and 0, and both again under VR_CLS_COLLAPSE=0 (the [CLS]-pooled BERTs only: nothing else
    reads that switch). Every output array of the four goes into OUT.npz. Run it under
    `rocprofv3 --kernel-trace --output-format csv -d DIR --`: every child leaves a trace of its own in DIR.

    The body: the models of tests/encoder_family_rows_case.py (FAMILIES x WIDTHS and Qwen2 at 896), the plain BERT of
    tests/test_encoder_rows_gpu.py at H = 768 (mean and CLS pooling), a Qwen3 model built with tests/test_qwen3_gpu.py's
    helpers (head size 128, Q/K norm, A = 512 over H = 256), the two models of tests/cls_collapse_case.py (large enough
    for `collapse` of forward_chunk to engage on its ladder batch) and one reranker. 3 layers, vocabulary 64 (the collapse
    models: their own 2 layers). Each in f16, f16x3 and f32, every call made twice (the second replays the cached graph
    where there is one), through encode and through encode_spans (every token a span), at FOLD_TOKENS and at
    span_batch(T) for T on both sides of 256 and of the first mid -> ping-pong change that family_route_edges gives for
    the device (the widest product's: 1280 / 1281 at H = 768, N = 4H on 256 CUs); [CLS]-pooled post-norm models also
    encode three_token_batch(n) for n = 256, 257 (the tail at M = n_seq).

python scripts/encoder_launch_sequence.py --compare DIR_A DIR_B A.npz B.npz
    search_launch_sequence.py's comparison of the two traces (launch count, multiset of (kernel, grid, workgroup), order
    per stream) and numpy.array_equal on every array, none with a non-finite value. Exit status 1 otherwise."""
import os
import subprocess
import sys

from search_launch_sequence import compare as compare_traces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = ("f16", "f16x3", "f32")
WAYS = {"fuse1": dict(VR_ENCODE_FUSE="1"), "fuse0": dict(VR_ENCODE_FUSE="0"),
        "fuse1-nocollapse": dict(VR_ENCODE_FUSE="1", VR_CLS_COLLAPSE="0"),
        "fuse0-nocollapse": dict(VR_ENCODE_FUSE="0", VR_CLS_COLLAPSE="0")}


def body(out_path, cls_only):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch

    import cls_collapse_case as cc
    import encoder_family_rows_case as fam
    import qwen3_oracle as q3
    import rerank_oracle as rr
    import test_qwen3_gpu as tq3
    from encoder_rows_case import mid_threshold, three_token_batch
    from oracle import bert as obert
    from test_encoder_rows_gpu import _Engine, _Oracle
    from voitta_rag_amd import Engine
    from voitta_rag_amd import encoder as enc

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    out = {}

    def keep(name, make):
        for rep in (1, 2):
            out[f"{name} #{rep}"] = np.asarray(make())

    def tokens(Ns):
        """FOLD_TOKENS, both sides of 256, both sides of the first mid -> ping-pong change among family_route_edges(Ns)."""
        thr = min((t for t in (mid_threshold(N, n_cu) for N in Ns) if t > 256), default=1024)
        assert {256, 257, thr, thr + 1} <= set(fam.family_route_edges(Ns, n_cu))
        return fam.FOLD_TOKENS + (256, 257, thr, thr + 1)

    def run(e, name, Ns, cls_tail):
        print(name, flush=True)
        for T in tokens(Ns):
            seqs, _ = fam.span_batch(T)
            keep(f"{name} encode T={T}", lambda: enc.encode(e, *fam.pack(seqs)))
            if not cls_tail:  # (a span call pools spans whatever the description says: the mean-pooled engine's route)
                keep(f"{name} encode_spans T={T}", lambda: enc.encode_spans(e, *fam.token_spans(seqs)))
        for n in (256, 257) if cls_tail else ():
            keep(f"{name} encode cls tail n={n}", lambda: enc.encode(e, *fam.pack(three_token_batch(n)[0])))

    bert = _Oracle("bge-base-en-v1.5")
    for precision in PRECISIONS:
        if not cls_only:
            for m in [fam.model(f, H) for f in fam.FAMILIES for H in fam.WIDTHS] + [fam.model("qwen2", 896)]:
                for pooling in ("mean",) if m.prenorm else ("mean", "cls"):
                    e = m.engine(pooling, precision)
                    run(e, f"{m.name} {pooling} {precision}", m.Ns, pooling == "cls")
                    e.close()
            shape = q3.Qwen3Shape(fam.LAYERS, 256, 4, 2, 512, 128, vocab=fam.VOCAB)
            e = tq3._engine(shape, "last", precision, q3.random_weights(shape, tq3.PATH_SEED), max_pos=fam.MAX_POS)
            run(e, f"qwen3 last {precision}", (shape.hidden, 3 * shape.attn, 2 * shape.intermediate), False)
            e.close()
            s = obert.BertShape(fam.LAYERS, 384, 6, 1536, vocab=fam.VOCAB, max_pos=fam.MAX_POS, type_vocab=2)
            e = Engine(s.hidden)
            enc.load_reranker(e, enc.BertDesc(s.layers, s.hidden, s.heads, s.intermediate, vocab=s.vocab, max_pos=s.max_pos,
                                              type_vocab=s.type_vocab, pooling="cls", normalize=False, eps=s.eps,
                                              precision=precision), rr.random_weights(s, 31, 40.0))
            for T in tokens((s.hidden, 3 * s.hidden, s.intermediate)):
                ids, off = fam.pack(fam.span_batch(T)[0])
                keep(f"reranker {precision} T={T}", lambda: e.rerank(ids, off, (np.diff(off) + 1) // 2))
            e.close()
        for pooling in ("cls",) if cls_only else ("mean", "cls"):
            with _Engine(bert, pooling, precision) as eng:
                s = bert.shape
                run(eng.e, f"bert-768 {pooling} {precision}", (s.hidden, 3 * s.hidden, s.intermediate), pooling == "cls")
        for dh in cc.HEAD_SIZES:
            m = cc.model(dh)
            e = cc.engine(m.shape, m.w, precision=precision, collapse=os.environ.get("VR_CLS_COLLAPSE") != "0")
            keep(f"{m.name} {precision} ladder", lambda: cc.encode(e, cc.ladder_batch()))
            e.close()
    np.savez(out_path, **out)


def run_ways(out_path):
    import numpy as np

    # every child opens the GPU for itself; this process never does (four at a time: well under any limit on GPU processes)
    children = [(way, f"{out_path}.{way}.npz",
                 subprocess.Popen([sys.executable, os.path.abspath(__file__), "--body", f"{out_path}.{way}.npz",
                                   "cls" if "VR_CLS_COLLAPSE" in env else "all"], env=dict(os.environ, **env)))
                for way, env in WAYS.items()]
    failed = [way for way, _, child in children if child.wait() != 0]
    if failed:
        sys.exit(f"failed: {failed}")
    merged = {}
    for way, part, _ in children:
        with np.load(part) as z:
            merged.update({f"{way}: {k}": z[k] for k in z.files})
        os.remove(part)
    np.savez(out_path, **merged)
    print(f"{len(merged)} arrays in {out_path}")


def compare_arrays(a, b):
    import numpy as np

    with np.load(a) as za, np.load(b) as zb:
        names = sorted(set(za.files) | set(zb.files))
        missing = [k for k in names if k not in za.files or k not in zb.files]
        different = [k for k in names if k not in missing and not np.array_equal(za[k], zb[k])]
        non_finite = [k for k in names for z in (za, zb) if k in z.files and not np.isfinite(z[k]).all()]
        rows = sum(len(za[k]) for k in za.files)
    print(f"arrays: {len(names)} ({rows} rows), on one side only {len(missing)}, different {len(different)}, "
          f"with a non-finite value {len(non_finite)}")
    for k in (missing + different + non_finite)[:40]:
        print("  ", k)
    return not (missing or different or non_finite)


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[1] == "--compare":
        same_launches = compare_traces(sys.argv[2], sys.argv[3])
        sys.exit(0 if compare_arrays(sys.argv[4], sys.argv[5]) and same_launches else 1)
    elif len(sys.argv) == 4 and sys.argv[1] == "--body":
        body(sys.argv[2], sys.argv[3] == "cls")
    elif len(sys.argv) == 2:
        run_ways(sys.argv[1])
    else:
        sys.exit(__doc__)
