#!/usr/bin/env python3
"""Terms aggregation with a metric on the device (tq_agg_terms_sub_batch_device: tq_agg_terms_sub.cpp,
tq_agg_terms_sub.hip; per key of a column its doc count and the stats of a second column, the top segment_size entries by
the metric's average).  The segment, key columns and batches are tools/bench_agg_terms.py's: Bitpacked Full key columns of
64, 2 048, 8 192 and 65 536 keys, UNIFORM and SKEWED, batches of `--queries` queries of four kinds (`+a +range` narrow and
wide, `*`, 2-term ORs); the metric column is a 20-bit Bitpacked Full "latency".  Order METRIC_DESC by AVG, segment_size
`--size`.  "timing" on, `--warmup` + `--reps` batches, the HIP-event kernel_ms of every timed batch.

Beside every row, FROM THE SAME RUN, the route of the code before this entry point: tq_agg_sub_batch_device with a
histogram of interval = gcd over the key column — one bucket per key, through f64 — its kernel_ms, and the bytes per query
each route puts on the bus: 64 + 44 x n_keys there (a host top-N follows), 40 + 52 x n_returned here.  The first eight
queries' rows are checked against a host top-N by exact average of that route's rows and records.

The byte model (include/tantivy_amd.h): tq_agg_terms_batch's + 8 per counted doc with a metric value + 40 x n_keys per
query + 40 per entry returned.  Records of a first measurement, not pass bars: no threshold is set or asserted.  The last
JSON line goes to profiles/agg_terms_sub_bench.json.

  python tools/bench_agg_terms_sub.py [--docs 10000000] [--terms 256] [--queries 1000] [--size 100] [--reps 10] [--warmup 2]
                                      [--keys 64,2048,8192,65536]"""
import argparse
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_agg_terms import HBM_PEAK_GBS, KEY_COUNTS, V_GCD, V_MIN, _say, _stat, make_key_column  # noqa: E402


def child(args):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from bench_range import make_columns
    from oracle import oracle as O
    import tantivy_amd as T
    from tests import column_model as CM

    B = T.binding
    seg = O.synth_segment(args.docs, n_terms=args.terms, with_positions=False)
    md = seg.max_doc
    dev = T.DeviceIndex([seg], devices=[0])
    dev.set_option("timing", 1)
    rng = np.random.default_rng(20261206)
    blob, t_vals = make_columns(md, rng)["bitpacked13"]
    col_t = dev.add_column(blob)  # the "timestamp" the range clauses are over
    col_m = dev.add_column(CM.write_bitpacked(rng.integers(0, 1 << 20, size=md).astype(np.uint64)))  # the "latency"
    columns = {}
    for n_keys in args.keys:
        for dist in ("uniform", "skewed"):
            blob, _ = make_key_column(md, n_keys, dist == "skewed", rng)
            columns[(n_keys, dist)] = dev.add_column(blob)
    caps = B.agg_terms_sub_lds_capacities()
    _say("segment and columns ready:", md, "docs; LDS capacities", caps)
    n, size = args.queries, args.size
    by_df = sorted(range(len(seg.terms)), key=lambda t: -seg.terms[t].doc_freq)
    terms = [by_df[i % len(by_df)] for i in range(n)]
    pairs = [t.tolist() for t in O.zipf_queries(n, 2, len(seg.terms), seed=11)]
    srt = np.sort(t_vals[:: max(1, t_vals.size // 100_000)])
    narrow, _ = dev.range_prepare(col_t, ("in", int(srt[srt.size // 2])), ("in", int(srt[min(srt.size - 1, srt.size // 2 + srt.size // 1000)])), 1.0)
    wide, _ = dev.range_prepare(col_t, ("in", int(srt[srt.size // 4])), ("in", int(srt[3 * srt.size // 4])), 1.0)
    kinds = {"must_a_must_range_narrow": [(T.MODE_AND, [a, narrow]) for a in terms],
             "must_a_must_range_wide": [(T.MODE_AND, [a, wide]) for a in terms],
             "star": [(T.MODE_BOOL, [B.TERM_ALL], [T.MUST], [0], 0)] * n,
             "or2": [(T.MODE_OR, p) for p in pairs]}
    dv = torch.device("cuda", 0)
    d_terms = torch.zeros(n * 5, dtype=torch.int64, device=dv)
    d_keys = torch.zeros(n * size, dtype=torch.int64, device=dv)
    d_counts = torch.zeros(n * size, dtype=torch.int32, device=dv)
    d_recs = torch.zeros(n * size * 5, dtype=torch.int64, device=dv)
    d_stats = torch.zeros(n * 8, dtype=torch.int64, device=dv)
    d_rows = torch.zeros(n * max(args.keys), dtype=torch.int32, device=dv)
    d_brecs = torch.zeros(n * max(args.keys) * 5, dtype=torch.int64, device=dv)
    out = {}

    def timed(run):
        """warm-up + timed batches of run() -> (kernel_ms list, the last batch's stats)"""
        ms, reps = [], args.reps
        for i in range(args.warmup + args.reps):
            assert run() == 0, B.lib().tq_last_error()
            st = dev.last_batch_stats()
            if i == 0 and st["kernel_ms"] > args.slow_ms:
                reps = min(args.reps, args.slow_reps)
            if i >= args.warmup:
                ms.append(st["kernel_ms"])
            if len(ms) >= reps:
                break
        return ms, st

    for (n_keys, dist), col in columns.items():
        width = min(size, n_keys)
        hist = {"interval": float(V_GCD), "offset": float(V_MIN)}
        assert dev.agg_terms_plan(col, B.TERMS_COUNT_DESC, size) == {"n_keys": n_keys, "min_value": V_MIN, "gcd": V_GCD}
        for kname, queries in kinds.items():
            h_ms, h_st = timed(lambda: dev.raw_agg_sub_device(queries, col, B.VALUE_U64, hist, col_m, B.VALUE_U64, n_keys, d_stats, d_rows, d_brecs))
            torch.cuda.synchronize(dv)
            head = d_rows[: 8 * n_keys].cpu().numpy().view(np.uint32).reshape(8, n_keys).astype(np.int64)
            head_recs = d_brecs[: 8 * n_keys * 5].cpu().numpy().view(np.uint64).reshape(8, n_keys, 5)
            ms, st = timed(lambda: dev.raw_agg_terms_sub_device(queries, col, col_m, B.VALUE_U64, B.TERMS_METRIC_DESC, size, B.METRIC_AVG, width,
                                                                d_terms, d_keys, d_counts, d_recs))
            torch.cuda.synchronize(dv)
            rec = d_terms.cpu().numpy().view(np.uint64)[: n * 5].view(B.AGG_TERMS_DTYPE)
            keys = d_keys.cpu().numpy().view(np.uint64)[: n * width].reshape(n, width)
            counts = d_counts.cpu().numpy().view(np.uint32)[: n * width].reshape(n, width)
            recs = d_recs.cpu().numpy().view(np.uint64)[: n * width * 5].reshape(n, width, 5)
            assert int(rec["out_of_range"].sum()) == 0 and int(st["matches"]) == int(h_st["matches"]) == int(rec["matches"].sum(dtype=np.uint64))
            for q in range(min(8, n)):  # the rows against a host top-N by exact average of the histogram route's rows
                nz = np.nonzero(head[q])[0].tolist()
                avg = {i: float(Fraction(int(head_recs[q, i, 3]) + (int(head_recs[q, i, 4]) << 64), int(head_recs[q, i, 0])))
                       if int(head_recs[q, i, 0]) else 0.0 for i in nz}
                top = sorted(nz, key=lambda i: (-avg[i], i))[:size]
                r = int(rec["n_returned"][q])
                assert r == len(top) and keys[q, :r].tolist() == [V_MIN + V_GCD * i for i in top], (n_keys, dist, kname, q)
                assert counts[q, :r].tolist() == [int(head[q][i]) for i in top] and int(rec["distinct"][q]) == len(nz)
                assert np.array_equal(recs[q, :r], head_recs[q][top]), (n_keys, dist, kname, q)
            med, h_med = float(np.median(ms)), float(np.median(h_ms))
            gbs = st["algorithmic_bytes"] / (med * 1e-3) / 1e9
            returned = int(rec["n_returned"].sum(dtype=np.uint64))
            out["%d_keys/%s/%s" % (n_keys, dist, kname)] = {
                "queries": n, "n_keys": n_keys, "segment_size": size, "matches": int(st["matches"]), "returned": returned,
                "accumulated_in": "lds" if n_keys <= caps[1] else "global", "kernels": st["kernels"],
                "terms_sub_kernel_ms": _stat(ms), "timed_batches": len(ms), "algorithmic_bytes": int(st["algorithmic_bytes"]),
                "implied_GBs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
                "histogram_sub_route_kernel_ms": _stat(h_ms), "histogram_sub_route_timed_batches": len(h_ms),
                "terms_sub_over_histogram_sub_route_ms": round(med / max(h_med, 1e-9), 3),
                "terms_sub_bus_bytes_per_query": round(40 + 52 * returned / n, 1), "histogram_sub_route_bus_bytes_per_query": 64 + 44 * n_keys}
            _say(n_keys, dist, kname, "terms_sub", round(med, 3), "ms, histogram sub route", round(h_med, 3), "ms")
    print("RESULT " + json.dumps({
        "docs": md, "terms": args.terms, "reps": args.reps, "warmup": args.warmup, "slow_ms": args.slow_ms, "slow_reps": args.slow_reps,
        "hbm_peak_GBs": HBM_PEAK_GBS, "order": "METRIC_DESC by AVG", "lds_capacities": list(caps),
        "byte_model": "tq_agg_terms_batch's + 8 per counted doc with a metric value + 40 x n_keys per query + 40 per entry returned",
        "note": "first measurement of this path: records, not pass bars; no threshold is set", "batches": out}))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--terms", type=int, default=256)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--size", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slow-ms", type=float, default=500.0, help="a batch slower than this in its first run ...")
    ap.add_argument("--slow-reps", type=int, default=3, help="... is timed this many times")
    ap.add_argument("--keys", type=lambda s: [int(x) for x in s.split(",")], default=list(KEY_COUNTS), help="the columns' key counts")
    ap.add_argument("--timeout", type=int, default=1100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agg_terms_sub_bench.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--docs", str(args.docs), "--terms", str(args.terms),
           "--queries", str(args.queries), "--size", str(args.size), "--reps", str(args.reps), "--warmup", str(args.warmup),
           "--slow-ms", str(args.slow_ms), "--slow-reps", str(args.slow_reps), "--keys", ",".join(str(k) for k in args.keys)]
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
        json.dump({"bench": "tools/bench_agg_terms_sub.py", "device": "MI355X", "result": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
