#!/usr/bin/env python3
"""Terms x histogram on the device (tq_agg_terms_hist_batch_device: tq_agg_terms_hist.cpp, tq_agg_terms_hist.hip; a dense
histogram of a second column per key of a terms aggregation).  On the synthetic segment of tools/bench_agg.py, the shapes of
the reference's four benchmarks of this collector (benches/agg_bench.rs):

  status_hist              7 skewed "status" keys x 120 hourly buckets of a u64 "timestamp"
  status_date_hist         the same over an I64 nanosecond date column (VALUE_I64)
  status_date_hist_bounds  ... under hard bounds that bind: the middle 60 hours
  zipf1000_hist            1 000 Zipf keys x 30 buckets

each with the docs TIME-SORTED (the timestamp rises with the doc id, as in an append-only log: the lanes of a wavefront
hold neighbouring docs, so with a low-cardinality key many of them add to one cell) and SHUFFLED.  Batches of `--queries`
queries of three kinds: `+a +range` over half of a 13-bit column, `*`, and 2-term ORs.  COUNT_DESC, segment_size `--size`.
"timing" on, `--warmup` + `--reps` batches, the HIP-event kernel_ms of every timed batch.

Beside every row, from the same run:
  * the A/B of LDS against global counting: the same batch with "agg_lds_buckets" = 0 (every add straight to the grid row);
  * the doc-set route of the code before this entry point, on the first `--baseline-queries` queries: tq_docset_batch_device
    rows (kernel_ms), their copy to the host, and the grid counted there with numpy from per-doc key and bucket arrays
    prepared once (np.bincount) — milliseconds per query, against this path's per query.  The device's rows of those
    queries are checked against that grid.

The byte model (include/tantivy_amd.h): tq_agg_terms_batch's + 8 per counted doc with a value in H + 4 x n_cells per query +
4 x n_buckets per entry returned.  Records of a first measurement, not pass bars.  The last JSON line goes to
profiles/agg_terms_hist_bench.json.

  python tools/bench_agg_terms_hist.py [--docs 4000000] [--terms 256] [--queries 256] [--size 100] [--reps 10] [--warmup 2]"""
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
HOURS = 120
TS_MIN = 472_222 * 3600  # (an hour's start)
DATE_MIN = (1 << 63) + TS_MIN * 10 ** 9  # an i64 of nanoseconds in the column's u64 space
NS = 10 ** 9


def _stat(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(np.min(xs)), 4), "max": round(float(np.max(xs)), 4)}


def _say(*a):
    sys.stderr.write(" ".join(str(x) for x in a) + "\n")
    sys.stderr.flush()


def _bitpacked(vmin, gcd, n, top):
    """A Bitpacked column of vmin + gcd * n, n <= top (rows 0 and the last pinned to 0 and top by the caller)."""
    from bench_range import _pack
    from tests import column_model as CM

    width = CM.compute_num_bits(top)
    blob = bytes([CM.BITPACKED]) + CM.stats_bytes(vmin, vmin + gcd * top, gcd, n.size) + _pack(n, width)
    for r in (0, 1, n.size // 2, n.size - 1):
        assert CM.read_one(blob, r) == vmin + gcd * int(n[r]), r
    return blob


def make_shapes(rows, rng):
    """name -> dict(t blob, t index per doc, h blob, bucket per doc (n_buckets: outside), value type, histogram, n_keys, n_buckets)"""
    seconds = np.sort(rng.integers(0, HOURS * 3600, size=rows)).astype(np.uint64)
    seconds[0], seconds[-1] = 0, HOURS * 3600 - 1
    status = rng.choice(7, size=rows, p=[0.55, 0.2, 0.1, 0.07, 0.05, 0.02, 0.01]).astype(np.uint64)
    status[0], status[-1] = 0, 6
    zipf = (rng.zipf(1.3, size=rows) % 1000).astype(np.uint64)
    zipf[0], zipf[-1] = 0, 999
    out = {}
    for order in ("time_sorted", "shuffled"):
        sec = seconds if order == "time_sorted" else seconds[rng.permutation(rows)]
        if order == "shuffled":
            sec[0], sec[-1] = 0, HOURS * 3600 - 1
        hour = (sec // np.uint64(3600)).astype(np.int64)
        h_u64, h_date = _bitpacked(TS_MIN, 1, sec, HOURS * 3600 - 1), _bitpacked(DATE_MIN, NS, sec, HOURS * 3600 - 1)
        t_status, t_zipf = _bitpacked(200, 100, status, 6), _bitpacked(1 << 40, 1, zipf, 999)
        # TS_MIN is a multiple of 3 600: the hourly buckets start on the column's minimum
        assert TS_MIN % 3600 == 0
        date_min_typed = float(TS_MIN * NS)
        inside = (hour >= 30) & (hour < 90)
        out["status_hist/" + order] = dict(t=t_status, t_idx=status, h=h_u64, bucket=hour, vt=0, hist={"interval": 3600.0},
                                           n_keys=7, n_buckets=HOURS)
        out["status_date_hist/" + order] = dict(t=t_status, t_idx=status, h=h_date, bucket=hour, vt=1, hist={"interval": 3600.0 * NS},
                                                n_keys=7, n_buckets=HOURS)
        out["status_date_hist_bounds/" + order] = dict(
            t=t_status, t_idx=status, h=h_date, bucket=np.where(inside, hour - 30, 60), vt=1,
            hist={"interval": 3600.0 * NS, "hard_bounds": (date_min_typed + 30 * 3600.0 * NS, date_min_typed + 90 * 3600.0 * NS - 1.0 * NS)},
            n_keys=7, n_buckets=60)
        out["zipf1000_hist/" + order] = dict(t=t_zipf, t_idx=zipf, h=h_u64, bucket=hour // 4, vt=0, hist={"interval": 4 * 3600.0, "offset": float(TS_MIN % (4 * 3600))},
                                             n_keys=1000, n_buckets=HOURS // 4)
    return out


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
    rng = np.random.default_rng(20261122)
    blob, r_vals = make_columns(md, rng)["bitpacked13"]
    col_r = dev.add_column(blob)  # the column the range clauses are over
    shapes = make_shapes(md, rng)
    caps = B.agg_terms_hist_lds_capacities()
    _say("segment and shapes ready:", md, "docs; LDS capacities", caps)
    n, size, nbase = args.queries, args.size, min(args.baseline_queries, args.queries)
    by_df = sorted(range(len(seg.terms)), key=lambda t: -seg.terms[t].doc_freq)
    terms = [by_df[i % len(by_df)] for i in range(n)]
    pairs = [t.tolist() for t in O.zipf_queries(n, 2, len(seg.terms), seed=11)]
    srt = np.sort(r_vals[:: max(1, r_vals.size // 100_000)])
    wide, _ = dev.range_prepare(col_r, ("in", int(srt[srt.size // 4])), ("in", int(srt[3 * srt.size // 4])), 1.0)
    kinds = {"must_a_must_range_wide": [(T.MODE_AND, [a, wide]) for a in terms],
             "star": [(T.MODE_BOOL, [B.TERM_ALL], [T.MUST], [0], 0)] * n,
             "or2": [(T.MODE_OR, p) for p in pairs]}
    dv = torch.device("cuda", 0)
    max_b = max(s["n_buckets"] for s in shapes.values())
    d_terms = torch.zeros(n * 5, dtype=torch.int64, device=dv)
    d_keys = torch.zeros(n * size, dtype=torch.int64, device=dv)
    d_counts = torch.zeros(n * size, dtype=torch.int32, device=dv)
    d_rows = torch.zeros(n * size * max_b, dtype=torch.int32, device=dv)
    d_docs = torch.zeros(nbase * md, dtype=torch.int32, device=dv)
    d_starts = torch.zeros(nbase + 1, dtype=torch.int64, device=dv)
    out = {}

    def timed(run):
        ms = []
        for i in range(args.warmup + args.reps):
            assert run() == 0, B.lib().tq_last_error()
            st = dev.last_batch_stats()
            if i >= args.warmup:
                ms.append(st["kernel_ms"])
        return ms, st

    handles = {}
    for name, sh in shapes.items():
        for k in ("t", "h"):
            if id(sh[k]) not in handles:
                handles[id(sh[k])] = dev.add_column(sh[k])
        ht, hh = handles[id(sh["t"])], handles[id(sh["h"])]
        nk, nb = sh["n_keys"], sh["n_buckets"]
        width = min(size, nk)
        plan = dev.agg_terms_hist_plan(ht, hh, sh["vt"], sh["hist"], B.TERMS_COUNT_DESC, size)
        assert (plan["terms"]["n_keys"], plan["hist"]["n_buckets"], plan["n_cells"]) == (nk, nb, nk * (nb + 1)), (name, plan)
        cell_of_doc = sh["t_idx"].astype(np.int64) * (nb + 1) + sh["bucket"]
        for kname, queries in kinds.items():
            def run():
                return dev.raw_agg_terms_hist_device(queries, ht, hh, sh["vt"], sh["hist"], B.TERMS_COUNT_DESC, size, width, nb,
                                                     d_terms, d_keys, d_counts, d_rows)

            ms, st = timed(run)
            torch.cuda.synchronize(dv)
            rec = d_terms.cpu().numpy().view(np.uint64)[: n * 5].view(B.AGG_TERMS_DTYPE).copy()
            keys = d_keys.cpu().numpy().view(np.uint64)[: n * width].reshape(n, width).copy()
            counts = d_counts.cpu().numpy().view(np.uint32)[: n * width].reshape(n, width).copy()
            rows = d_rows.cpu().numpy().view(np.uint32)[: n * width * nb].reshape(n, width, nb).copy()
            assert int(rec["out_of_range"].sum()) == 0 and st["kernel_mask"] == B.KERNEL_AGG_TERMS_HIST
            dev.set_option("agg_lds_buckets", 0)  # the A/B: every add straight to the grid row
            g_ms, _ = timed(run)
            dev.set_option("agg_lds_buckets", caps[1])
            torch.cuda.synchronize(dv)
            assert np.array_equal(rec, d_terms.cpu().numpy().view(np.uint64)[: n * 5].view(B.AGG_TERMS_DTYPE))
            # the doc-set route on the first queries: rows, their copy, the grid on the host
            base = queries[:nbase]
            ds_ms, ds_st = timed(lambda: dev.raw_docset_device(base, d_docs, nbase * md, d_starts))
            torch.cuda.synchronize(dv)
            t0 = time.perf_counter()
            starts = d_starts.cpu().numpy().view(np.uint64)
            docs = d_docs[: int(starts[nbase])].cpu().numpy().view(np.uint32)
            t1 = time.perf_counter()
            grids = [np.bincount(cell_of_doc[docs[int(starts[q]): int(starts[q + 1])]], minlength=nk * (nb + 1)).reshape(nk, nb + 1)
                     for q in range(nbase)]
            t2 = time.perf_counter()
            for q in range(nbase):  # the device's rows against the host's grid
                total = grids[q].sum(axis=1)
                nz = np.nonzero(total)[0]
                top = nz[np.lexsort((nz, -total[nz]))][:size]
                r = int(rec["n_returned"][q])
                assert r == top.size and keys[q, :r].tolist() == [plan["terms"]["min_value"] + plan["terms"]["gcd"] * int(i) for i in top], (name, kname, q)
                assert counts[q, :r].tolist() == total[top].tolist() and np.array_equal(rows[q, :r], grids[q][top, :nb]), (name, kname, q)
            med, g_med = float(np.median(ms)), float(np.median(g_ms))
            gbs = st["algorithmic_bytes"] / (med * 1e-3) / 1e9
            route = {"docset_kernel_ms": float(np.median(ds_ms)) / nbase, "copy_ms": (t1 - t0) * 1e3 / nbase, "host_count_ms": (t2 - t1) * 1e3 / nbase}
            route_total = sum(route.values())
            out["%s/%s" % (name, kname)] = {
                "queries": n, "n_keys": nk, "n_buckets": nb, "n_cells": nk * (nb + 1), "segment_size": size, "matches": int(st["matches"]),
                "returned": int(rec["n_returned"].sum(dtype=np.uint64)), "counted_in": "lds" if nk * (nb + 1) <= caps[1] else "global",
                "kernels": st["kernels"], "kernel_ms": _stat(ms), "kernel_ms_global_counting": _stat(g_ms),
                "lds_over_global_ms": round(med / max(g_med, 1e-9), 3), "algorithmic_bytes": int(st["algorithmic_bytes"]),
                "implied_GBs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4), "ms_per_query": round(med / n, 5),
                "docset_route_queries": nbase, "docset_route_ms_per_query": {k: round(v, 4) for k, v in route.items()},
                "docset_route_total_ms_per_query": round(route_total, 4), "speedup_over_docset_route": round(route_total / max(med / n, 1e-9), 1)}
            _say(name, kname, "device", round(med, 3), "ms (global counting", round(g_med, 3), "ms); doc-set route", round(route_total, 3), "ms per query")
    print("RESULT " + json.dumps({
        "docs": md, "terms": args.terms, "reps": args.reps, "warmup": args.warmup, "hbm_peak_GBs": HBM_PEAK_GBS, "order": "COUNT_DESC",
        "lds_capacities": list(caps),
        "byte_model": "tq_agg_terms_batch's + 8 per counted doc with a value in H + 4 x n_cells per query + 4 x n_buckets per entry returned",
        "note": "first measurement of this path: records, not pass bars", "batches": out}))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=4_000_000)
    ap.add_argument("--terms", type=int, default=256)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--baseline-queries", type=int, default=8, help="queries of every batch that also go the doc-set route")
    ap.add_argument("--size", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=1100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agg_terms_hist_bench.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--docs", str(args.docs), "--terms", str(args.terms),
           "--queries", str(args.queries), "--baseline-queries", str(args.baseline_queries), "--size", str(args.size),
           "--reps", str(args.reps), "--warmup", str(args.warmup)]
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
        json.dump({"bench": "tools/bench_agg_terms_hist.py", "device": "MI355X", "result": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
