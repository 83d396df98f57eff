#!/usr/bin/env python
"""Multi-field segments on the device (tq_segment_upload_fields; tree_fields_kernel): one 10 M-doc segment of two Zipf
fields — t(itle) = field 0, the primary field, b(ody) = field 1 — from the oracle's generator (two independent
segments over one doc-id space: another seed, its own fieldnorms).

  batches   1 000 queries with k = 10 of the shapes QueryParser makes of `a b` over the default fields [t, b],
              should   (t:a b:a) (t:b b:b)
              must     +(t:a b:a) +(t:b b:b)
            and, for comparison with the primary path (shared / pruned kernels on the same lists' primary-field twins),
              primary  +t:a +t:b        (TQ_MODE_AND over field 0: the headline's shape, pruned)
              body     +b:a +b:b        (the same over field 1: tree_fields_kernel, nothing pruned)
            through tq_search_batch: kernel ms from tq_last_batch_stats (option "timing"), the kernel families, the
            HBM model's bytes over the median as a fraction of 8 TB/s.

Protocol: 2 warm-up runs, then 10 timed runs of every call; median [min .. max].  Nothing could run the multi-field
shapes before: there is no threshold, this is the record.  The parent starts one child process under a time limit; the
JSON line goes to profiles/fields_bench.json.

  python tools/bench_fields.py [--docs 10000000] [--terms 8192] [--queries 1000] [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
SHAPES = ("should", "must", "primary", "body")


def _stat(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(np.min(xs)), 4), "max": round(float(np.max(xs)), 4)}


def child(args):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from oracle import oracle as O
    import tantivy_amd as T

    M, S = T.MUST, T.SHOULD
    fields = [O.synth_segment(args.docs, n_terms=args.terms, segment_ord=f, with_positions=False) for f in (0, 1)]
    dev = T.DeviceIndex(devices=[0])
    base = dev.add_segment_fields(fields)
    dev.set_option("timing", 1)
    n, k = args.queries, 10
    pairs = [q.tolist() for q in O.zipf_queries(n, 2, min(256, args.terms), seed=20261019)]
    md = fields[0].max_doc
    avgs = [f.avg_fieldnorm for f in fields]
    cache = np.stack([np.array(list(O.bm25_for_one_term(1, md, a).cache), np.float32) for a in avgs])
    w = lambda f, t: float(O.bm25_for_one_term(fields[f].terms[t].doc_freq, md, avgs[f]).weight)  # noqa: E731
    g = lambda f, t: base[f] + t  # noqa: E731
    shapes = {
        "should": [((T.MODE_BOOL, [g(0, a), g(1, a), g(0, b), g(1, b)], None, [S] * 4, [0, 0, 1, 1], 0), [w(0, a), w(1, a), w(0, b), w(1, b)])
                   for a, b in pairs],
        "must": [((T.MODE_BOOL, [g(0, a), g(1, a), g(0, b), g(1, b)], None, [M] * 4, [0, 0, 1, 1], 0), [w(0, a), w(1, a), w(0, b), w(1, b)])
                 for a, b in pairs],
        "primary": [((T.MODE_AND, [g(0, a), g(0, b)], None), [w(0, a), w(0, b)]) for a, b in pairs],
        "body": [((T.MODE_AND, [g(1, a), g(1, b)], None), [w(1, a), w(1, b)]) for a, b in pairs],
    }
    results = {}
    for name in SHAPES:
        qs = [x[0] for x in shapes[name]]
        ws = [x[1] for x in shapes[name]]
        ms = []
        for i in range(args.warmup + args.reps):
            dev.raw_search(qs, ws, cache, k)
            st = dev.last_batch_stats()
            if i >= args.warmup:
                ms.append(st["kernel_ms"])
        med = float(np.median(ms))
        results[name] = {"queries": n, "k": k, "kernels": st["kernels"], "kernel_ms": _stat(ms),
                         "algorithmic_bytes": int(st["algorithmic_bytes"]), "matches": int(st["matches"]),
                         "model_frac_of_peak": round(st["algorithmic_bytes"] / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    assert results["should"]["kernels"] == ["tree"] and results["body"]["kernels"] == ["tree"], results
    assert "tree" not in results["primary"]["kernels"], results
    print("RESULT " + json.dumps({"docs": args.docs, "terms": args.terms, "fields": 2, "reps": args.reps, "warmup": args.warmup,
                                  "hbm_peak_GBs": HBM_PEAK_GBS, "fields_stats": dev.fields_stats(),
                                  "segment_stats": dev.segment_stats(), "shapes": results}))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--terms", type=int, default=8192)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fields_bench.json"))
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
        json.dump({"bench": "tools/bench_fields.py", "device": "MI355X", "result": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
