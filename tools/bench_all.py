#!/usr/bin/env python
"""AllQuery clauses on the device (TQ_TERM_ALL: tq_all.hip for the top-k, the doc-set passes for counts and doc sets):
a 10 M-doc Zipf segment from the oracle's generator, batches of 1 000 queries with k = 10 of the four everyday shapes

  star        *                     every doc, score 1
  all_not     +* -a                 everything but
  all_opt     +* a b                every doc, boosted where a or b hit
  all_min1    * a b  (minimum 1)    the docs of a or b, score s + 1

each through tq_search_batch (kernel ms from tq_last_batch_stats, option "timing"), tq_count_batch (wall ms of the C call: it
ends in a synchronise) and tq_docset_scored_batch_device (kernel ms; the batch cut so that its rows stay under 4 GB).
For context the same `a b` pairs as plain unions with "exhaustive" = 1 through today's path.  Protocol: warm-up runs,
then `reps` timed runs of every call; median, minimum and maximum are reported, and the HBM model's bytes
(tq_batch_stats.algorithmic_bytes) over the median as a fraction of 8 TB/s.

The parent starts one child process under a time limit; the JSON line goes to profiles/all_bench.json.

  python tools/bench_all.py [--docs 10000000] [--queries 1000] [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
OUT_BYTES_MAX = 4 << 30
SHAPES = ("star", "all_not", "all_opt", "all_min1")


def _stat(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(np.min(xs)), 4), "max": round(float(np.max(xs)), 4)}


def child(args):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from oracle import oracle as O
    import tantivy_amd as T

    B = T.binding
    ALL, M, S, N = B.TERM_ALL, T.MUST, T.SHOULD, T.MUST_NOT
    seg = O.synth_segment(args.docs, n_terms=args.terms, with_positions=False)
    dev = T.DeviceIndex([seg], devices=[0])
    dev.set_option("timing", 1)
    n, k = args.queries, 10
    pairs = [q.tolist() for q in O.zipf_queries(n, 2, args.terms, seed=20261018)]
    avg = seg.avg_fieldnorm
    w_of = {t: float(O.bm25_for_one_term(seg.terms[t].doc_freq, seg.max_doc, avg).weight) for p in pairs for t in p}
    cache = np.array(list(O.bm25_for_one_term(1, seg.max_doc, avg).cache), np.float32)
    # (search tuple, flat tuple, weights) per shape
    shapes = {
        "star": [((T.MODE_OR, [ALL]), (T.MODE_OR, [ALL]), [1.0]) for _ in pairs],
        "all_not": [((T.MODE_BOOL, [ALL, a], None, [M, N], None, 0), (T.MODE_BOOL, [ALL, a], [M, N], None, 0), [1.0, w_of[a]])
                    for a, _ in pairs],
        "all_opt": [((T.MODE_BOOL, [ALL, a, b], None, [M, S, S], None, 0), (T.MODE_BOOL, [ALL, a, b], [M, S, S], None, 0),
                     [1.0, w_of[a], w_of[b]]) for a, b in pairs],
        "all_min1": [((T.MODE_BOOL, [ALL, a, b], None, [S, S, S], None, 1), (T.MODE_BOOL, [ALL, a, b], [S, S, S], None, 1),
                      [1.0, w_of[a], w_of[b]]) for a, b in pairs],
    }
    stream = torch.cuda.Stream()
    results = {}
    for name in SHAPES:
        sq = [x[0] for x in shapes[name]]
        fq = [x[1] for x in shapes[name]]
        ws = [x[2] for x in shapes[name]]
        # top-k
        ms = []
        for i in range(args.warmup + args.reps):
            sc, dc, ct = dev.raw_search(sq, ws, cache, k, opts=(1, 0))
            st = dev.last_batch_stats()
            if i >= args.warmup:
                ms.append(st["kernel_ms"])
        assert st["kernels"] == ["all"], st
        sizes = dev.last_batch_match_counts(n)
        if name == "star":
            assert np.all(dc == np.arange(k, dtype=np.uint32)) and np.all(sc == 1.0) and np.all(sizes == seg.max_doc)
        # Count
        cw = []
        qs, keep = dev._raw_scored_queries(fq, ws, cache, 0)  # marshalled once: the timed region is the C call alone
        counts = np.zeros(n, np.uint32)
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            B._check(B.lib().tq_count_batch(dev.segment_raw(0), qs, n, B._u32(counts)))
            if i >= args.warmup:
                cw.append((time.perf_counter() - t0) * 1e3)
        count_kernels = dev.last_batch_stats()["kernels"]
        assert np.array_equal(counts, sizes), name  # the doc set's size, the number the exhaustive search reports
        # scored doc sets: as many queries as keep docs + scores under the limit
        n_ds = int(np.searchsorted(np.cumsum(counts.astype(np.int64)) * 8, OUT_BYTES_MAX, side="right"))
        n_ds = max(1, min(n, n_ds))
        total = int(counts[:n_ds].astype(np.int64).sum())
        d_docs = torch.empty(max(1, total), dtype=torch.int32, device="cuda")
        d_scores = torch.empty(max(1, total), dtype=torch.float32, device="cuda")
        d_starts = torch.zeros(n_ds + 1, dtype=torch.int64, device="cuda")
        ds = []
        for i in range(args.warmup + args.reps):
            rc = dev.raw_docset_scored_device(fq[:n_ds], d_docs, d_scores, total, d_starts, stream=stream.cuda_stream,
                                              weights=ws[:n_ds], cache=cache)
            assert rc == 0, B.lib().tq_last_error()
            dst = dev.last_batch_stats()
            if i >= args.warmup:
                ds.append(dst["kernel_ms"])
        assert int(d_starts[-1].item()) == total and dst["matches"] == total
        del d_docs, d_scores, d_starts
        med = float(np.median(ms))
        results[name] = {
            "queries": n, "k": k, "search_kernel_ms": _stat(ms), "search_algorithmic_bytes": int(st["algorithmic_bytes"]),
            "search_model_GBs": round(st["algorithmic_bytes"] / (med * 1e-3) / 1e9, 1),
            "search_model_frac_of_peak": round(st["algorithmic_bytes"] / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "search_tiles": int(st["tiles"]), "docs_in_sets": int(sizes.astype(np.int64).sum()), "docs_scored": int(st["matches"]),
            "count_wall_ms": _stat(cw), "count_kernels": count_kernels,
            "docset_scored_queries": n_ds, "docset_scored_docs": total, "docset_scored_kernel_ms": _stat(ds),
            "docset_scored_algorithmic_bytes": int(dst["algorithmic_bytes"]),
            "docset_scored_model_frac_of_peak": round(dst["algorithmic_bytes"] / (float(np.median(ds)) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
        }
    # context: the same pairs as plain unions, every match scored, through today's path
    uq = [(T.MODE_OR, p) for p in pairs]
    uw = [[w_of[a], w_of[b]] for a, b in pairs]
    ms = []
    for i in range(args.warmup + args.reps):
        dev.raw_search(uq, uw, cache, k, opts=(1, 0))
        st = dev.last_batch_stats()
        if i >= args.warmup:
            ms.append(st["kernel_ms"])
    results["union_exhaustive_context"] = {"queries": n, "k": k, "search_kernel_ms": _stat(ms), "kernels": st["kernels"],
                                           "search_algorithmic_bytes": int(st["algorithmic_bytes"]), "matches": int(st["matches"])}
    print("RESULT " + json.dumps({"docs": args.docs, "terms": args.terms, "reps": args.reps, "warmup": args.warmup,
                                  "hbm_peak_GBs": HBM_PEAK_GBS, "shapes": results}))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--terms", type=int, default=256)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "all_bench.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--docs", str(args.docs), "--terms", str(args.terms),
           "--queries", str(args.queries), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        raise SystemExit("no result after %d s: stopping" % args.timeout)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("failed (exit %d)" % r.returncode)
    res = json.loads(line[-1][7:])
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"bench": "tools/bench_all.py", "device": "MI355X", "result": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
