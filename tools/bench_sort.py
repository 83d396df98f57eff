#!/usr/bin/env python3
"""Sort by fast field on the device (tq_search_sorted_batch_device: tq_sort.cpp, tq_sort.hip;
TopDocs::order_by_fast_field).  On one synthetic segment, sorted by a 13-bit Bitpacked Full column and by an Optional one
with half of the docs holding a value, batches of `--queries` queries of four kinds — `+a +range` with a narrow (about
0.1 % of the value span) and a wide (about 50 %) range over the sort column, `*`, and 2-term ORs — at k = 10 and 1024,
descending with nulls last.  "timing" on, `--warmup` + `--reps` batches, the HIP-event kernel_ms of every timed batch.

Beside every batch, in the same run, what serves the request without this entry point: tq_docset_batch_device over the
same queries (its kernel_ms; the rows would then go down the bus, 4 bytes per matching doc, and be sorted on the host).
Its output buffer is capped at `--docset-cap` docs — the passes run in full, stores past the cap are dropped — so for the
batches that match more than that its time is a LOWER bound.

The byte model of a sorted batch (include/tantivy_amd.h): every list's bitmap words once + 8 per matching doc with a value
+ 8 per matching doc of an Optional column + 13 per row entry.  GB/s is that model over the event time, against the
8 TB/s HBM figure bench.py's roofline uses.  These are records of a first measurement, not pass bars.  The last JSON line
goes to profiles/sort_bench.json.

  python tools/bench_sort.py [--docs 10000000] [--terms 256] [--queries 1000] [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK_GBS = 8000.0  # bench.py's roofline figure


def _stat(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(np.min(xs)), 4), "max": round(float(np.max(xs)), 4)}


def child(args):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from bench_range import make_columns
    from oracle import oracle as O
    from tests import column_model as CM
    import tantivy_amd as T

    B = T.binding
    seg = O.synth_segment(args.docs, n_terms=args.terms, with_positions=False)
    md = seg.max_doc
    dev = T.DeviceIndex([seg], devices=[0])
    dev.set_option("timing", 1)
    rng = np.random.default_rng(20261019)
    blob, vals = make_columns(md, rng)["bitpacked13"]
    present = rng.random(md) < 0.5
    oblob, ovals = make_columns(int(present.sum()), rng)["bitpacked13"]
    columns = {"bitpacked13": (dev.add_column(blob), vals), "bitpacked13_optional":
               (dev.add_column(oblob, CM.OPTIONAL, CM.presence_words(present)), ovals)}
    n = args.queries
    by_df = sorted(range(len(seg.terms)), key=lambda t: -seg.terms[t].doc_freq)
    terms = [by_df[i % len(by_df)] for i in range(n)]
    pairs = [t.tolist() for t in O.zipf_queries(n, 2, len(seg.terms), seed=11)]
    dv = torch.device("cuda", 0)
    stride = 1024
    d_docs = torch.zeros(n * stride, dtype=torch.int32, device=dv)
    d_vals = torch.zeros(n * stride, dtype=torch.int64, device=dv)
    d_has = torch.zeros(n * stride, dtype=torch.uint8, device=dv)
    d_cnt = torch.zeros(n, dtype=torch.int32, device=dv)
    d_set = torch.zeros(args.docset_cap, dtype=torch.int32, device=dv)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dv)
    out = {}
    for cname, (col, cvals) in columns.items():
        srt = np.sort(cvals[:: max(1, cvals.size // 100_000)])
        mid = int(srt[srt.size // 2])
        narrow, _ = dev.range_prepare(col, ("in", mid), ("in", int(srt[min(srt.size - 1, srt.size // 2 + srt.size // 1000)])), 1.0)
        wide, _ = dev.range_prepare(col, ("in", int(srt[srt.size // 4])), ("in", int(srt[3 * srt.size // 4])), 1.0)
        kinds = {"must_a_must_range_narrow": [(T.MODE_AND, [a, narrow]) for a in terms],
                 "must_a_must_range_wide": [(T.MODE_AND, [a, wide]) for a in terms],
                 "star": [(T.MODE_BOOL, [B.TERM_ALL], [T.MUST], [0], 0)] * n,
                 "or2": [(T.MODE_OR, p) for p in pairs]}
        for kname, queries in kinds.items():
            # what serves the request without the sorted call: the doc sets
            ds_ms = []
            for i in range(args.warmup + args.reps):
                rc = dev.raw_docset_device(queries, d_set, args.docset_cap, d_starts)
                assert rc == 0, B.lib().tq_last_error()
                st = dev.last_batch_stats()
                if i >= args.warmup:
                    ds_ms.append(st["kernel_ms"])
            matches = int(st["matches"])
            for k in (10, 1024):
                ms = []
                for i in range(args.warmup + args.reps):
                    rc = dev.raw_search_sorted_device(queries, col, B.SORT_DESC, B.NULLS_LAST, k, stride, d_docs, d_vals, d_has, d_cnt)
                    assert rc == 0, B.lib().tq_last_error()
                    st = dev.last_batch_stats()
                    if i >= args.warmup:
                        ms.append(st["kernel_ms"])
                assert int(st["matches"]) == matches, (cname, kname, k)
                med = float(np.median(ms))
                gbs = st["algorithmic_bytes"] / (med * 1e-3) / 1e9
                out["%s/%s/k%d" % (cname, kname, k)] = {
                    "queries": n, "k": k, "matches": matches, "kernels": st["kernels"], "sorted_kernel_ms": _stat(ms),
                    "algorithmic_bytes": int(st["algorithmic_bytes"]), "implied_GBs": round(gbs, 1),
                    "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4), "docset_kernel_ms": _stat(ds_ms),
                    "docset_time_is_lower_bound": matches > args.docset_cap, "docset_bus_bytes": 4 * matches,
                    "sorted_bus_bytes": 13 * n * k, "docset_over_sorted_ms": round(float(np.median(ds_ms)) / max(med, 1e-9), 3)}
        for h in (narrow, wide):
            dev.term_set_release(h)
    print("RESULT " + json.dumps({
        "docs": md, "terms": args.terms, "reps": args.reps, "warmup": args.warmup, "hbm_peak_GBs": HBM_PEAK_GBS,
        "docset_cap": args.docset_cap, "order": "descending, nulls last",
        "byte_model": "lists x bitmap words x 4 + 8 per valued match + 8 per match of an Optional column + 13 per row entry",
        "note": "first measurement of this path: records, not pass bars", "batches": out}))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--terms", type=int, default=256)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--docset-cap", type=int, default=1 << 26)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sort_bench.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--docs", str(args.docs), "--terms", str(args.terms),
           "--queries", str(args.queries), "--reps", str(args.reps), "--warmup", str(args.warmup), "--docset-cap", str(args.docset_cap)]
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
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"bench": "tools/bench_sort.py", "device": "MI355X", "result": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
