#!/usr/bin/env python3
"""Sub-aggregations on the device (tq_agg_sub_batch_device: tq_agg.cpp, tq_agg_sub.hip; a histogram over a bucket column A
with the stats of a metric column B per bucket).  On one synthetic segment, A = a 13-bit Bitpacked Full column, B = a second
13-bit column — Full, and Optional with half of the docs holding a value — batches of `--queries` queries of the four kinds
of tools/bench_agg.py (`+a +range` narrow and wide over A, `*`, 2-term ORs), at 64 buckets and at one bucket more than the
capacity of each of the kernel's two LDS tables (the large table; the global path).  "timing" on, `--warmup` + `--reps`
batches, the HIP-event kernel_ms of every timed batch.

Beside every row, from the same run:
  * tq_agg_batch_device over the same queries and the same histogram without the metric — what the second column adds to
    the walk;
  * tq_docset_batch_device over the same queries — the route that serves the request without this entry point: its
    kernel_ms, and the 4 bytes per matching doc that then go down the bus to a host loop over two host copies of columns.
    Its output buffer is capped at `--docset-cap` docs (the passes run in full, stores past the cap are dropped), so for the
    batches that match more than that its time is a LOWER bound.

The byte model (include/tantivy_amd.h): tq_agg_batch's for A + 8 per bucketed doc with a value in B + 8 per bucketed doc of
an Optional B + 40 x n_buckets per query.  Records of a first measurement, not pass bars.  The last JSON line goes to
profiles/agg_sub_bench.json.

`--ab`: the A/B of LDS table sizes — B Full, `*` and the 2-term ORs, 64 buckets alone; `--variant` labels the library
measured (TQ_LIB_PATH chooses it, tools/build_variant.py builds it).

  python tools/bench_agg_sub.py [--docs 10000000] [--terms 256] [--queries 1000] [--reps 10] [--warmup 2] [--ab]"""
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
V_MIN, V_GCD = 1 << 40, 1000  # the 13-bit columns of bench_range.make_columns: V_MIN + V_GCD * n, n < 8192


def _stat(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(np.min(xs)), 4), "max": round(float(np.max(xs)), 4)}


def _say(*a):
    sys.stderr.write(" ".join(str(x) for x in a) + "\n")
    sys.stderr.flush()


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
    rng = np.random.default_rng(20261022)
    blob, a_vals = make_columns(md, rng)["bitpacked13"]
    col_a = dev.add_column(blob)
    metrics = {"full": dev.add_column(make_columns(md, rng)["bitpacked13"][0])}
    if not args.ab:
        present = rng.random(md) < 0.5
        metrics["optional"] = dev.add_column(make_columns(int(present.sum()), rng)["bitpacked13"][0], CM.OPTIONAL, CM.presence_words(present))
    small_cap, large_cap = B.agg_sub_lds_capacities()
    _say("segment and columns ready:", md, "docs; LDS capacities", small_cap, large_cap)

    def past(c):  # interval 1 (packed value) under hard bounds: c + 1 buckets
        return {"interval": 1.0 * V_GCD, "offset": float(V_MIN), "hard_bounds": (float(V_MIN), float(V_MIN + c * V_GCD))}

    modes = {"hist64": ({"interval": 128.0 * V_GCD, "offset": float(V_MIN)}, 64)}
    if not args.ab:
        modes["small_cap_plus_1"] = (past(small_cap), small_cap + 1)
        modes["large_cap_plus_1"] = (past(large_cap), large_cap + 1)
    n = args.queries
    by_df = sorted(range(len(seg.terms)), key=lambda t: -seg.terms[t].doc_freq)
    terms = [by_df[i % len(by_df)] for i in range(n)]
    pairs = [t.tolist() for t in O.zipf_queries(n, 2, len(seg.terms), seed=11)]
    srt = np.sort(a_vals[:: max(1, a_vals.size // 100_000)])
    narrow, _ = dev.range_prepare(col_a, ("in", int(srt[srt.size // 2])), ("in", int(srt[min(srt.size - 1, srt.size // 2 + srt.size // 1000)])), 1.0)
    wide, _ = dev.range_prepare(col_a, ("in", int(srt[srt.size // 4])), ("in", int(srt[3 * srt.size // 4])), 1.0)
    kinds = {"must_a_must_range_narrow": [(T.MODE_AND, [a, narrow]) for a in terms],
             "must_a_must_range_wide": [(T.MODE_AND, [a, wide]) for a in terms],
             "star": [(T.MODE_BOOL, [B.TERM_ALL], [T.MUST], [0], 0)] * n,
             "or2": [(T.MODE_OR, p) for p in pairs]}
    if args.ab:
        kinds = {k: kinds[k] for k in ("star", "or2")}
    max_nb = max(nb for _, nb in modes.values())
    dv = torch.device("cuda", 0)
    d_stats = torch.zeros(n * 8, dtype=torch.int64, device=dv)
    d_rows = torch.zeros(n * max_nb, dtype=torch.int32, device=dv)
    d_recs = torch.zeros(n * max_nb * 5, dtype=torch.int64, device=dv)
    d_set = torch.zeros(args.docset_cap, dtype=torch.int32, device=dv)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dv)
    info = dev.column_info(col_a)
    out = {}
    for kname, queries in kinds.items():
        ds_ms = []  # the route without this entry point: the doc sets
        for i in range(args.warmup + args.reps):
            rc = dev.raw_docset_device(queries, d_set, args.docset_cap, d_starts)
            assert rc == 0, B.lib().tq_last_error()
            st = dev.last_batch_stats()
            if i >= args.warmup:
                ds_ms.append(st["kernel_ms"])
        matches = int(st["matches"])
        for mname, (hist, want_nb) in modes.items():
            nb = B.agg_histogram_plan(info, B.VALUE_U64, hist["interval"], hist["offset"], hist.get("hard_bounds"))["n_buckets"]
            assert nb == want_nb, (mname, nb)
            agg_ms = []  # the histogram alone
            for i in range(args.warmup + args.reps):
                rc = dev.raw_agg_device(queries, col_a, B.VALUE_U64, hist, nb, d_stats, d_rows)
                assert rc == 0, B.lib().tq_last_error()
                st = dev.last_batch_stats()
                if i >= args.warmup:
                    agg_ms.append(st["kernel_ms"])
            torch.cuda.synchronize(dv)
            agg_rows = d_rows.cpu().numpy().view(np.uint32)[: n * nb].reshape(n, nb).copy()
            for bname, col_b in metrics.items():
                ms = []
                for i in range(args.warmup + args.reps):
                    rc = dev.raw_agg_sub_device(queries, col_a, B.VALUE_U64, hist, col_b, B.VALUE_U64, nb, d_stats, d_rows, d_recs)
                    assert rc == 0, B.lib().tq_last_error()
                    st = dev.last_batch_stats()
                    if i >= args.warmup:
                        ms.append(st["kernel_ms"])
                assert int(st["matches"]) == matches, (kname, mname, bname)
                torch.cuda.synchronize(dv)
                rec = d_stats.cpu().numpy().view(np.uint64)[: n * 8].view(B.AGG_STATS_DTYPE)
                rows = d_rows.cpu().numpy().view(np.uint32)[: n * nb].reshape(n, nb)
                recs = d_recs.cpu().numpy().view(np.uint64)[: n * nb * 5].view(B.AGG_BUCKET_STATS_DTYPE).reshape(n, nb)
                assert int(rec["out_of_range"].sum()) == 0 and np.array_equal(rows, agg_rows), (kname, mname, bname)
                assert np.all(recs["count"] <= rows) and (bname != "full" or np.array_equal(recs["count"], rows)), (kname, mname, bname)
                med = float(np.median(ms))
                gbs = st["algorithmic_bytes"] / (med * 1e-3) / 1e9
                out["%s/%s/%s" % (bname, kname, mname)] = {
                    "queries": n, "n_buckets": nb, "matches": matches, "bucketed": int(rows.sum(dtype=np.uint64)),
                    "bucketed_with_metric_value": int(recs["count"].sum(dtype=np.uint64)), "kernels": st["kernels"],
                    "agg_sub_kernel_ms": _stat(ms), "algorithmic_bytes": int(st["algorithmic_bytes"]), "implied_GBs": round(gbs, 1),
                    "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4), "agg_histogram_alone_kernel_ms": _stat(agg_ms),
                    "sub_over_histogram_alone": round(med / max(float(np.median(agg_ms)), 1e-9), 3),
                    "docset_kernel_ms": _stat(ds_ms), "docset_time_is_lower_bound": matches > args.docset_cap,
                    "docset_bus_bytes": 4 * matches, "agg_sub_bus_bytes": n * (64 + 44 * nb),
                    "docset_over_sub_ms": round(float(np.median(ds_ms)) / max(med, 1e-9), 3)}
                _say(bname, kname, mname, "sub", round(med, 3), "ms, histogram alone", round(float(np.median(agg_ms)), 3), "ms, doc sets",
                     round(float(np.median(ds_ms)), 3), "ms")
    print("RESULT " + json.dumps({
        "docs": md, "terms": args.terms, "reps": args.reps, "warmup": args.warmup, "hbm_peak_GBs": HBM_PEAK_GBS,
        "docset_cap": args.docset_cap, "variant": args.variant, "lds_capacities": [small_cap, large_cap],
        "byte_model": "tq_agg_batch's for A + 8 per bucketed doc with a B value + 8 per bucketed doc of an Optional B + 40 x n_buckets per query",
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
    ap.add_argument("--ab", action="store_true", help="the A/B of LDS table sizes: B Full, `*` and or2, 64 buckets")
    ap.add_argument("--variant", default="stock", help="a label for the library measured (TQ_LIB_PATH chooses it)")
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agg_sub_bench.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--docs", str(args.docs), "--terms", str(args.terms),
           "--queries", str(args.queries), "--reps", str(args.reps), "--warmup", str(args.warmup), "--docset-cap", str(args.docset_cap),
           "--variant", args.variant] + (["--ab"] if args.ab else [])
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
        json.dump({"bench": "tools/bench_agg_sub.py", "device": "MI355X", "result": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
