#!/usr/bin/env python3
"""Range aggregation on the device (tq_agg_range_batch_device: tq_agg_range.cpp, tq_agg_range.hip; doc counts per range of a
bucket column A, alone or with the stats of a metric column B per range).  On one synthetic segment, A = a 13-bit Bitpacked
Full column, B = a second one, batches of `--queries` queries of the four kinds of tools/bench_agg.py (`+a +range` narrow and
wide over A, `*`, 2-term ORs), at 4, 64 and 1 024 buckets — the most a request may have, which is also the large capacity of
the kernel's record table, so "one more than the capacity" does not exist as a request — and at 1 024 buckets once more
with "agg_lds_buckets" = 16: the global path.  "timing" on, `--warmup` + `--reps` batches, the HIP-event kernel_ms of every
timed batch: median (min - max).

Beside every row, from the same run:
  * tq_agg_batch_device / tq_agg_sub_batch_device with a HISTOGRAM of the same number of equal-width buckets over the same
    queries — what the search over the starts costs against one f64 division;
  * the route a caller has without this entry point: one tq_range_prepare + one tq_count_batch of `q AND range` per range.
    Measured on at most `--route-ranges` of the ranges (evenly spaced; prepare + count wall time and the count's kernel_ms
    each) and SCALED to the number of ranges: `route_scaled` says whether the figure is measured in full or extrapolated.

The byte model (include/tantivy_amd.h): tq_agg_batch's for A with this n_buckets + 8 x n_buckets per call + with a metric
tq_agg_sub_batch's terms for B.  Records of a first measurement, not pass bars: nothing here is asserted about a time.  The
last JSON line goes to profiles/agg_range_bench.json.

  python tools/bench_agg_range.py [--docs 10000000] [--terms 256] [--queries 1000] [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import subprocess
import sys
import time

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
    import tantivy_amd as T

    B = T.binding
    seg = O.synth_segment(args.docs, n_terms=args.terms, with_positions=False)
    md = seg.max_doc
    dev = T.DeviceIndex([seg], devices=[0])
    dev.set_option("timing", 1)
    rng = np.random.default_rng(20261023)
    blob, a_vals = make_columns(md, rng)["bitpacked13"]
    col_a = dev.add_column(blob)
    col_b = dev.add_column(make_columns(md, rng)["bitpacked13"][0])
    small_cap, large_cap = B.agg_range_lds_capacities()
    _say("segment and columns ready:", md, "docs; record-table capacities", small_cap, large_cap)

    def mode(nb):
        """nb equal-width buckets over the 8 192 packed values of A: the user ranges (the first one open below, the last one
        open above, so the plan inserts nothing) and the histogram with the same edges"""
        interval = 8192.0 * V_GCD / nb  # (a whole number of packed values for 4 and 64 buckets)
        edges = [float(V_MIN) + interval * i for i in range(nb)]
        ranges = [(None, edges[1])] + [(edges[i], edges[i + 1]) for i in range(1, nb - 1)] + [(edges[nb - 1], None)]
        return ranges, {"interval": interval, "offset": float(V_MIN)}, edges

    modes = {"range4": 4, "range64": 64, "range1024": B.AGG_RANGE_MAX_BUCKETS}
    n = args.queries
    by_df = sorted(range(len(seg.terms)), key=lambda t: -seg.terms[t].doc_freq)
    terms = [by_df[i % len(by_df)] for i in range(n)]
    pairs = [t.tolist() for t in O.zipf_queries(n, 2, len(seg.terms), seed=11)]
    srt = np.sort(a_vals[:: max(1, a_vals.size // 100_000)])
    narrow, _ = dev.range_prepare(col_a, ("in", int(srt[srt.size // 2])), ("in", int(srt[min(srt.size - 1, srt.size // 2 + srt.size // 1000)])), 1.0)
    wide, _ = dev.range_prepare(col_a, ("in", int(srt[srt.size // 4])), ("in", int(srt[3 * srt.size // 4])), 1.0)
    M = T.MUST
    # (the aggregation's query, how the same query reads with one more Must clause `r` for tq_count_batch)
    kinds = {"must_a_must_range_narrow": ([(T.MODE_AND, [a, narrow]) for a in terms], lambda r: [(T.MODE_AND, [a, narrow, r]) for a in terms]),
             "must_a_must_range_wide": ([(T.MODE_AND, [a, wide]) for a in terms], lambda r: [(T.MODE_AND, [a, wide, r]) for a in terms]),
             "star": ([(T.MODE_BOOL, [B.TERM_ALL], [M], [0], 0)] * n, lambda r: [(T.MODE_AND, [r])] * n),
             "or2": ([(T.MODE_OR, p) for p in pairs], lambda r: [(T.MODE_BOOL, p + [r], None, [M, M, M], [0, 0, 1], 0) for p in pairs])}
    max_nb = max(modes.values())
    dv = torch.device("cuda", 0)
    d_stats = torch.zeros(n * 8, dtype=torch.int64, device=dv)
    d_rows = torch.zeros(n * max_nb, dtype=torch.int32, device=dv)
    d_recs = torch.zeros(n * max_nb * 5, dtype=torch.int64, device=dv)
    info = dev.column_info(col_a)
    cache = np.ones(256, np.float32)
    out = {}

    def timed(call):
        ms = []
        for i in range(args.warmup + args.reps):
            rc = call()
            assert rc == 0, B.lib().tq_last_error()
            st = dev.last_batch_stats()
            if i >= args.warmup:
                ms.append(st["kernel_ms"])
        return ms, st

    for kname, (queries, with_range) in kinds.items():
        for mname, nb in modes.items():
            ranges, hist, edges = mode(nb)
            plan = B.agg_range_plan(B.VALUE_U64, ranges)
            hnb = B.agg_histogram_plan(info, B.VALUE_U64, hist["interval"], hist["offset"])["n_buckets"]
            assert len(plan) == nb and hnb == nb, (mname, len(plan), hnb)
            # the route of today: one range clause and one count batch per range, on a sample of the ranges
            sample = sorted(set(np.linspace(0, nb - 1, min(nb, args.route_ranges)).astype(int).tolist()))
            route_wall, route_kernel = [], []
            for i in sample:
                t0 = time.perf_counter()
                lower = None if i == 0 else ("in", int(edges[i]))
                upper = None if i == nb - 1 else ("ex", int(edges[i + 1]))
                h, _ = dev.range_prepare(col_a, lower, upper, 1.0)
                qs = with_range(h)
                dev.raw_count(qs, [[1.0] * len(q[1]) for q in qs], cache)
                route_wall.append((time.perf_counter() - t0) * 1e3)
                route_kernel.append(dev.last_batch_stats()["kernel_ms"])
            for metric in (False, True):
                if metric:
                    base_ms, _ = timed(lambda: dev.raw_agg_sub_device(queries, col_a, B.VALUE_U64, hist, col_b, B.VALUE_U64, nb, d_stats, d_rows, d_recs))
                else:
                    base_ms, _ = timed(lambda: dev.raw_agg_device(queries, col_a, B.VALUE_U64, hist, nb, d_stats, d_rows))
                torch.cuda.synchronize(dv)
                hist_rows = d_rows.cpu().numpy().view(np.uint32)[: n * nb].reshape(n, nb).copy()
                ms, st = timed(lambda: dev.raw_agg_range_device(queries, col_a, B.VALUE_U64, ranges, col_b if metric else None,
                                                                B.VALUE_U64, nb, d_stats, d_rows, d_recs if metric else None))
                torch.cuda.synchronize(dv)
                rec = d_stats.cpu().numpy().view(np.uint64)[: n * 8].view(B.AGG_STATS_DTYPE)
                rows = d_rows.cpu().numpy().view(np.uint32)[: n * nb].reshape(n, nb)
                # equal-width ranges ARE the histogram's buckets: the same docs, and where the edges are whole numbers the same
                # rows, from another kernel (a fractional edge is truncated by the range's conversion, not by the histogram)
                assert int(rec["out_of_range"].sum()) == 0 and int(rows.sum(dtype=np.uint64)) == int(hist_rows.sum(dtype=np.uint64))
                assert (8192 * V_GCD) % nb or np.array_equal(rows, hist_rows), (kname, mname, metric)
                med = float(np.median(ms))
                gbs = st["algorithmic_bytes"] / (med * 1e-3) / 1e9
                scale = nb / len(sample)
                out["%s/%s/%s" % ("metric" if metric else "counts", kname, mname)] = {
                    "queries": n, "n_buckets": nb, "matches": int(st["matches"]), "bucketed": int(rows.sum(dtype=np.uint64)),
                    "kernels": st["kernels"], "agg_range_kernel_ms": _stat(ms), "algorithmic_bytes": int(st["algorithmic_bytes"]),
                    "implied_GBs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
                    "histogram_same_buckets_kernel_ms": _stat(base_ms),
                    "range_over_histogram": round(med / max(float(np.median(base_ms)), 1e-9), 3),
                    "route_ranges_measured": len(sample), "route_scaled": len(sample) < nb,
                    "route_per_range_wall_ms": _stat(route_wall), "route_per_range_count_kernel_ms": _stat(route_kernel),
                    "route_all_ranges_wall_ms": round(float(np.sum(route_wall)) * scale, 3),
                    "route_all_ranges_count_kernel_ms": round(float(np.sum(route_kernel)) * scale, 3),
                    "route_kernel_over_range_ms": round(float(np.sum(route_kernel)) * scale / max(med, 1e-9), 2)}
                _say("metric" if metric else "counts", kname, mname, "range", round(med, 3), "ms, histogram", round(float(np.median(base_ms)), 3),
                     "ms, per-range route", round(float(np.sum(route_wall)) * scale, 1), "ms of wall time")
                if nb == B.AGG_RANGE_MAX_BUCKETS:  # the same request past "agg_lds_buckets": atomics on the query's rows
                    dev.set_option("agg_lds_buckets", 16)
                    gms, gst = timed(lambda: dev.raw_agg_range_device(queries, col_a, B.VALUE_U64, ranges, col_b if metric else None,
                                                                      B.VALUE_U64, nb, d_stats, d_rows, d_recs if metric else None))
                    dev.set_option("agg_lds_buckets", 8192)
                    torch.cuda.synchronize(dv)
                    assert np.array_equal(d_rows.cpu().numpy().view(np.uint32)[: n * nb].reshape(n, nb), hist_rows) or (8192 * V_GCD) % nb
                    out["%s/%s/%s_global_path" % ("metric" if metric else "counts", kname, mname)] = {
                        "queries": n, "n_buckets": nb, "agg_lds_buckets": 16, "agg_range_kernel_ms": _stat(gms),
                        "global_over_lds": round(float(np.median(gms)) / max(med, 1e-9), 3)}
                    _say("   ... past agg_lds_buckets:", round(float(np.median(gms)), 3), "ms")
    print("RESULT " + json.dumps({
        "docs": md, "terms": args.terms, "reps": args.reps, "warmup": args.warmup, "hbm_peak_GBs": HBM_PEAK_GBS,
        "lds_capacities": [small_cap, large_cap], "route_ranges": args.route_ranges,
        "byte_model": "tq_agg_batch's for A with this n_buckets + 8 x n_buckets per call + with a metric: 8 per bucketed doc with a B value + 8 per bucketed doc of an Optional B + 40 x n_buckets per query",
        "note": "first measurement of this path: records, not pass bars", "batches": out}))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--terms", type=int, default=256)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--route-ranges", type=int, default=4, help="ranges of a request the per-range route is measured on")
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agg_range_bench.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--docs", str(args.docs), "--terms", str(args.terms),
           "--queries", str(args.queries), "--reps", str(args.reps), "--warmup", str(args.warmup), "--route-ranges", str(args.route_ranges)]
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
        json.dump({"bench": "tools/bench_agg_range.py", "device": "MI355X", "result": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
