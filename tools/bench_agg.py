#!/usr/bin/env python3
"""Aggregations over a fast field on the device (tq_agg_batch_device: tq_agg.cpp, tq_agg.hip; a stats metric and a
histogram).  On one synthetic segment, over a 13-bit Bitpacked Full column and an Optional one with half of the docs holding
a value, batches of `--queries` queries of four kinds — `+a +range` with a narrow (about 0.1 % of the value span) and a wide
(about 50 %) range over the aggregated column, `*`, and 2-term ORs — in three modes: stats alone, a 64-bucket histogram and
an 8 192-bucket histogram.  A third, SKEWED Full column holds one value in 90 % of its docs: its 64-bucket histogram puts
nine docs of ten into one bucket.  "timing" on, `--warmup` + `--reps` batches, the HIP-event kernel_ms of every timed batch.

Beside every batch, in the same run, what serves the request without this entry point: tq_docset_batch_device over the
same queries (its kernel_ms; the rows would then go down the bus, 4 bytes per matching doc, and be aggregated by a host loop
over a host copy of the column).  Its output buffer is capped at `--docset-cap` docs — the passes run in full, stores past
the cap are dropped — so for the batches that match more than that its time is a LOWER bound.

The byte model of an aggregation batch (include/tantivy_amd.h): every list's bitmap words once + 8 per matching doc with a
value + 8 per matching doc of an Optional column + 64 + 4 x n_buckets per query.  GB/s is that model over the event time,
against the 8 TB/s HBM figure bench.py's roofline uses.  These are records of a first measurement, not pass bars.  The
last JSON line goes to profiles/agg_bench.json.

  python tools/bench_agg.py [--docs 10000000] [--terms 256] [--queries 1000] [--reps 10] [--warmup 2] [--only-skewed]"""
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
V_MIN, V_GCD = 1 << 40, 1000


def _stat(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(np.min(xs)), 4), "max": round(float(np.max(xs)), 4)}


def _say(*a):
    sys.stderr.write(" ".join(str(x) for x in a) + "\n")
    sys.stderr.flush()


def child(args):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from bench_range import _pack, make_columns
    from oracle import oracle as O
    from tests import column_model as CM
    import tantivy_amd as T

    B = T.binding
    seg = O.synth_segment(args.docs, n_terms=args.terms, with_positions=False)
    md = seg.max_doc
    dev = T.DeviceIndex([seg], devices=[0])
    dev.set_option("timing", 1)
    if args.lds_buckets >= 0:
        dev.set_option("agg_lds_buckets", args.lds_buckets)
    rng = np.random.default_rng(20261021)
    columns = {}
    if not args.only_skewed:
        blob, vals = make_columns(md, rng)["bitpacked13"]
        present = rng.random(md) < 0.5
        oblob, ovals = make_columns(int(present.sum()), rng)["bitpacked13"]
        columns["bitpacked13"] = (dev.add_column(blob), vals)
        columns["bitpacked13_optional"] = (dev.add_column(oblob, CM.OPTIONAL, CM.presence_words(present)), ovals)
    # the skewed column: 90 % of the docs hold packed value 4096, the others are uniform
    n_sk = rng.integers(0, 1 << 13, size=md).astype(np.uint64)
    n_sk[rng.random(md) < 0.9] = 4096
    n_sk[0], n_sk[-1] = 0, (1 << 13) - 1
    sblob = bytes([CM.BITPACKED]) + CM.stats_bytes(V_MIN, V_MIN + V_GCD * 8191, V_GCD, md) + _pack(n_sk, 13)
    columns["bitpacked13_skewed"] = (dev.add_column(sblob), np.uint64(V_MIN) + np.uint64(V_GCD) * n_sk)
    _say("segment and columns ready:", md, "docs")
    # histograms over [V_MIN, V_MIN + 8 191 000]: one bucket per packed value, and one per 128 of them
    modes = {"stats": None, "hist64": {"interval": 128.0 * V_GCD, "offset": float(V_MIN)},
             "hist8192": {"interval": 1.0 * V_GCD, "offset": float(V_MIN)}}
    n = args.queries
    by_df = sorted(range(len(seg.terms)), key=lambda t: -seg.terms[t].doc_freq)
    terms = [by_df[i % len(by_df)] for i in range(n)]
    pairs = [t.tolist() for t in O.zipf_queries(n, 2, len(seg.terms), seed=11)]
    dv = torch.device("cuda", 0)
    d_stats = torch.zeros(n * 8, dtype=torch.int64, device=dv)
    d_rows = torch.zeros(n * 8192, dtype=torch.int32, device=dv)
    d_set = torch.zeros(args.docset_cap, dtype=torch.int32, device=dv)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dv)
    out = {}
    for cname, (col, cvals) in columns.items():
        skewed = cname.endswith("skewed")
        srt = np.sort(cvals[:: max(1, cvals.size // 100_000)])
        mid = int(srt[srt.size // 2])
        narrow, _ = dev.range_prepare(col, ("in", mid), ("in", int(srt[min(srt.size - 1, srt.size // 2 + srt.size // 1000)])), 1.0)
        wide, _ = dev.range_prepare(col, ("in", int(srt[srt.size // 4])), ("in", int(srt[3 * srt.size // 4])), 1.0)
        kinds = {"must_a_must_range_narrow": [(T.MODE_AND, [a, narrow]) for a in terms],
                 "must_a_must_range_wide": [(T.MODE_AND, [a, wide]) for a in terms],
                 "star": [(T.MODE_BOOL, [B.TERM_ALL], [T.MUST], [0], 0)] * n,
                 "or2": [(T.MODE_OR, p) for p in pairs]}
        if skewed:
            kinds = {k: kinds[k] for k in ("star", "or2")}
        for kname, queries in kinds.items():
            # what serves the request without the aggregation call: the doc sets
            ds_ms = []
            for i in range(args.warmup + args.reps):
                rc = dev.raw_docset_device(queries, d_set, args.docset_cap, d_starts)
                assert rc == 0, B.lib().tq_last_error()
                st = dev.last_batch_stats()
                if i >= args.warmup:
                    ds_ms.append(st["kernel_ms"])
            matches = int(st["matches"])
            for mname, hist in modes.items():
                if skewed and mname == "stats":
                    continue
                info = dev.column_info(col)
                nb = B.agg_histogram_plan(info, B.VALUE_U64, hist["interval"], hist["offset"])["n_buckets"] if hist else 0
                assert nb == {"stats": 0, "hist64": 64, "hist8192": 8192}[mname], (mname, nb)
                ms = []
                for i in range(args.warmup + args.reps):
                    rc = dev.raw_agg_device(queries, col, B.VALUE_U64, hist, nb, d_stats, d_rows if nb else None)
                    assert rc == 0, B.lib().tq_last_error()
                    st = dev.last_batch_stats()
                    if i >= args.warmup:
                        ms.append(st["kernel_ms"])
                assert int(st["matches"]) == matches, (cname, kname, mname)
                torch.cuda.synchronize(dv)
                rec = d_stats.cpu().numpy().view(np.uint64)[: n * 8].view(B.AGG_STATS_DTYPE)
                assert int(rec["matches"].astype(object).sum()) == matches and int(rec["out_of_range"].sum()) == 0
                if nb:
                    rows = d_rows.cpu().numpy().view(np.uint32)[: n * nb].reshape(n, nb)
                    assert np.array_equal(rows.sum(axis=1, dtype=np.uint64), rec["in_bounds"]), (cname, kname, mname)
                    hot = float(rows[0].max()) / max(1.0, float(rows[0].sum()))
                med = float(np.median(ms))
                gbs = st["algorithmic_bytes"] / (med * 1e-3) / 1e9
                out["%s/%s/%s" % (cname, kname, mname)] = {
                    "queries": n, "n_buckets": nb, "matches": matches, "kernels": st["kernels"], "agg_kernel_ms": _stat(ms),
                    "algorithmic_bytes": int(st["algorithmic_bytes"]), "implied_GBs": round(gbs, 1),
                    "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4), "docset_kernel_ms": _stat(ds_ms),
                    "docset_time_is_lower_bound": matches > args.docset_cap, "docset_bus_bytes": 4 * matches,
                    "agg_bus_bytes": n * (64 + 4 * nb), "docset_over_agg_ms": round(float(np.median(ds_ms)) / max(med, 1e-9), 3)}
                if nb:
                    out["%s/%s/%s" % (cname, kname, mname)]["hottest_bucket_share_query0"] = round(hot, 3)
                _say(cname, kname, mname, "agg", round(med, 3), "ms, doc sets", round(float(np.median(ds_ms)), 3), "ms")
        for h in (narrow, wide):
            dev.term_set_release(h)
    print("RESULT " + json.dumps({
        "docs": md, "terms": args.terms, "reps": args.reps, "warmup": args.warmup, "hbm_peak_GBs": HBM_PEAK_GBS,
        "docset_cap": args.docset_cap, "variant": args.variant, "agg_lds_buckets": args.lds_buckets if args.lds_buckets >= 0 else "default",
        "byte_model": "lists x bitmap words x 4 + 8 per valued match + 8 per match of an Optional column + (64 + 4 x n_buckets) per query",
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
    ap.add_argument("--only-skewed", action="store_true", help="the skewed column alone (A/B runs of a kernel variant)")
    ap.add_argument("--lds-buckets", type=int, default=-1, help='option "agg_lds_buckets" (default: the capacity of the LDS table)')
    ap.add_argument("--variant", default="stock", help="a label for the library measured (TQ_LIB_PATH chooses it)")
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agg_bench.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--docs", str(args.docs), "--terms", str(args.terms),
           "--queries", str(args.queries), "--reps", str(args.reps), "--warmup", str(args.warmup), "--docset-cap", str(args.docset_cap),
           "--variant", args.variant, "--lds-buckets", str(args.lds_buckets)] + (["--only-skewed"] if args.only_skewed else [])
    try:
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=args.timeout)  # (progress: its stderr)
    except subprocess.TimeoutExpired:
        raise SystemExit("no result after %d s: stopping" % args.timeout)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:])
        raise SystemExit("failed (exit %d)" % r.returncode)
    res = json.loads(line[-1][7:])
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"bench": "tools/bench_agg.py", "device": "MI355X", "result": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
