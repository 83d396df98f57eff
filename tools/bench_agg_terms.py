#!/usr/bin/env python3
"""Terms aggregation on the device (tq_agg_terms_batch_device: tq_agg_terms.cpp, tq_agg_terms.hip; the top segment_size
values of a fast-field column by doc count).  On the synthetic segment of tools/bench_agg.py, over Bitpacked Full columns of
64, 2 048, 8 192 and 65 536 keys (V_MIN + V_GCD * n) — UNIFORM, and SKEWED with nine docs of ten in one key — batches of
`--queries` queries of that tool's four kinds: `+a +range` with a narrow (about 0.1 % of the span) and a wide (about 50 %)
range over a 13-bit "timestamp" column, `*`, and 2-term ORs.  COUNT_DESC, segment_size `--size`.  "timing" on, `--warmup` +
`--reps` batches, the HIP-event kernel_ms of every timed batch (a batch whose warm-up run takes more than `--slow-ms` is
timed `--slow-reps` times; the row says so).

Beside every row, from the same run, the route of the code before this entry point: tq_agg_batch_device with a histogram of
interval = gcd over the same column — one bucket per key, through f64 — its kernel_ms, and the bytes per query each route
puts on the bus: 64 + 4 x n_keys there (a host top-N follows), 40 + 12 x n_returned here.  The first eight queries' rows are
checked against a top-N of that histogram's rows.

The byte model (include/tantivy_amd.h): every list's bitmap words once + 8 per matching doc with a value + (40 + 4 x n_keys)
per query + 12 per entry returned.  Records of a first measurement, not pass bars.  The last JSON line goes to
profiles/agg_terms_bench.json.

`--keys 65536 --variant LABEL` with TQ_LIB_PATH and `tools/build_variant.py LABEL tq_agg_terms.hip
-DTQ_AGG_TERMS_GLOBAL_TABLE=<entries>` is the A/B of profiles/agg_terms_global_ab.txt: which instantiation the global path
runs in.

  python tools/bench_agg_terms.py [--docs 10000000] [--terms 256] [--queries 1000] [--size 100] [--reps 10] [--warmup 2]
                                  [--keys 64,2048,8192,65536] [--variant LABEL]"""
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
KEY_COUNTS = (64, 2048, 8192, 65536)


def _stat(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(np.min(xs)), 4), "max": round(float(np.max(xs)), 4)}


def _say(*a):
    sys.stderr.write(" ".join(str(x) for x in a) + "\n")
    sys.stderr.flush()


def make_key_column(rows, n_keys, skewed, rng):
    """-> (blob, key indices): a Bitpacked column of V_MIN + V_GCD * n, n below n_keys; skewed: nine rows of ten hold the
    middle key."""
    from bench_range import _pack
    from tests import column_model as CM

    n = rng.integers(0, n_keys, size=rows).astype(np.uint64)
    if skewed:
        n[rng.random(rows) < 0.9] = n_keys // 2
    n[0], n[-1] = 0, n_keys - 1
    width = CM.compute_num_bits(n_keys - 1)
    blob = bytes([CM.BITPACKED]) + CM.stats_bytes(V_MIN, V_MIN + V_GCD * (n_keys - 1), V_GCD, rows) + _pack(n, width)
    for r in (0, 1, rows // 2, rows - 1):
        assert CM.read_one(blob, r) == V_MIN + V_GCD * int(n[r]), (n_keys, r)
    return blob, n


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
    rng = np.random.default_rng(20261103)
    blob, t_vals = make_columns(md, rng)["bitpacked13"]
    col_t = dev.add_column(blob)  # the "timestamp" the range clauses are over
    columns = {}
    for n_keys in args.keys:
        for dist in ("uniform", "skewed"):
            blob, _ = make_key_column(md, n_keys, dist == "skewed", rng)
            columns[(n_keys, dist)] = dev.add_column(blob)
    caps = B.agg_terms_lds_capacities()
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
    d_stats = torch.zeros(n * 8, dtype=torch.int64, device=dv)
    d_rows = torch.zeros(n * max(args.keys), dtype=torch.int32, device=dv)
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
        assert B.agg_histogram_plan(dev.column_info(col), B.VALUE_U64, hist["interval"], hist["offset"])["n_buckets"] == n_keys
        for kname, queries in kinds.items():
            h_ms, h_st = timed(lambda: dev.raw_agg_device(queries, col, B.VALUE_U64, hist, n_keys, d_stats, d_rows))
            torch.cuda.synchronize(dv)
            rows = d_rows.cpu().numpy().view(np.uint32)[: n * n_keys].reshape(n, n_keys)
            row_sums = rows.sum(axis=1, dtype=np.uint64)
            head = rows[:8].astype(np.int64)
            ms, st = timed(lambda: dev.raw_agg_terms_device(queries, col, B.TERMS_COUNT_DESC, size, width, d_terms, d_keys, d_counts))
            torch.cuda.synchronize(dv)
            rec = d_terms.cpu().numpy().view(np.uint64)[: n * 5].view(B.AGG_TERMS_DTYPE)
            keys = d_keys.cpu().numpy().view(np.uint64)[: n * width].reshape(n, width)
            counts = d_counts.cpu().numpy().view(np.uint32)[: n * width].reshape(n, width)
            assert int(rec["out_of_range"].sum()) == 0 and np.array_equal(rec["count"], row_sums), (n_keys, dist, kname)
            assert int(st["matches"]) == int(h_st["matches"]) == int(rec["matches"].sum(dtype=np.uint64))
            for q in range(min(8, n)):  # the rows against a host top-N of the histogram route's row
                nz = np.nonzero(head[q])[0]
                top = nz[np.lexsort((nz, -head[q][nz]))][:size]
                r = int(rec["n_returned"][q])
                assert r == top.size and keys[q, :r].tolist() == [V_MIN + V_GCD * int(i) for i in top], (n_keys, dist, kname, q)
                assert counts[q, :r].tolist() == head[q][top].tolist() and int(rec["distinct"][q]) == nz.size
            med, h_med = float(np.median(ms)), float(np.median(h_ms))
            gbs = st["algorithmic_bytes"] / (med * 1e-3) / 1e9
            returned = int(rec["n_returned"].sum(dtype=np.uint64))
            out["%d_keys/%s/%s" % (n_keys, dist, kname)] = {
                "queries": n, "n_keys": n_keys, "segment_size": size, "matches": int(st["matches"]), "returned": returned,
                "counted_in": "lds" if n_keys <= caps[1] else "global", "kernels": st["kernels"],
                "terms_kernel_ms": _stat(ms), "timed_batches": len(ms), "algorithmic_bytes": int(st["algorithmic_bytes"]),
                "implied_GBs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
                "histogram_route_kernel_ms": _stat(h_ms), "histogram_route_timed_batches": len(h_ms),
                "terms_over_histogram_route_ms": round(med / max(h_med, 1e-9), 3),
                "terms_bus_bytes_per_query": round(40 + 12 * returned / n, 1), "histogram_route_bus_bytes_per_query": 64 + 4 * n_keys}
            _say(n_keys, dist, kname, "terms", round(med, 3), "ms, histogram route", round(h_med, 3), "ms")
    print("RESULT " + json.dumps({
        "docs": md, "terms": args.terms, "reps": args.reps, "warmup": args.warmup, "slow_ms": args.slow_ms, "slow_reps": args.slow_reps,
        "hbm_peak_GBs": HBM_PEAK_GBS, "order": "COUNT_DESC", "lds_capacities": list(caps), "variant": args.variant,
        "byte_model": "bitmap words + 8 per valued matching doc + (40 + 4 x n_keys) per query + 12 per entry returned",
        "note": "first measurement of this path: records, not pass bars", "batches": out}))
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
    ap.add_argument("--variant", default="stock", help="a label for the library measured (TQ_LIB_PATH chooses it)")
    ap.add_argument("--timeout", type=int, default=1100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agg_terms_bench.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--docs", str(args.docs), "--terms", str(args.terms),
           "--queries", str(args.queries), "--size", str(args.size), "--reps", str(args.reps), "--warmup", str(args.warmup),
           "--slow-ms", str(args.slow_ms), "--slow-reps", str(args.slow_reps), "--keys", ",".join(str(k) for k in args.keys),
           "--variant", args.variant]
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
        json.dump({"bench": "tools/bench_agg_terms.py", "device": "MI355X", "result": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
