#!/usr/bin/env python3
"""Fast-field range clauses on the device (tq_range_prepare: tq_column.cpp, tq_range.hip; a RangeQuery on a u64 fast field
as a const-score bitmap).  On one synthetic segment, per codec (Bitpacked 13 bits, Linear 6-bit diffs, BlockwiseLinear
11-bit diffs; a Full column, and the Bitpacked one again as an Optional column of half the docs) at a narrow (about 0.1 %
of the value span) and a wide (about 50 %) range:
  build     "timing": tq_range_prepare brackets the zeroing, the fill and the rank stage with two HIP events and leaves the
            time and the byte model in tq_batch_stats — kernel_ms, algorithmic_bytes, and from them the implied GB/s
  batches   `+a +range` for `--queries` terms a through tq_search_batch (HIP-event kernel_ms of the batch) and
            tq_count_batch (wall time of the C call)
The byte model of a build: the column's payload read once + 16 B per 32 docs (the table written by the fill and the scan,
read once by the scan) + 8 B per 32 docs of presence table for an Optional column.  GB/s and the fraction of peak are that
model over the event time against the 8 TB/s HBM figure bench.py's roofline uses.  These are records of a first
measurement, not pass bars: there is no earlier number for this path.  The columns' bytes are written by vectorised
writers below (any valid Line is a valid column; tests/column_model.py's reader checks a sample of rows).  The last JSON
line goes to profiles/range_bench.json.

  python tools/bench_range.py [--docs 10000000] [--terms 256] [--queries 200] [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0  # bench.py's roofline figure


def _stat(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(np.min(xs)), 4), "max": round(float(np.max(xs)), 4)}


def _pack(ns, width):
    """The reference's bit packer over a uint64 array, a million rows at a time."""
    out = []
    for i in range(0, ns.size, 1 << 20):
        a = ns[i: i + (1 << 20)]
        bits = ((a[:, None] >> np.arange(width, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
        out.append(np.packbits(bits.reshape(-1), bitorder="little").tobytes())
    return b"".join(out)


def make_columns(rows, rng):
    """name -> (blob, values): one column per codec over `rows` rows."""
    from tests import column_model as CM

    cols = {}
    n = rng.integers(0, 1 << 13, size=rows).astype(np.uint64)
    n[0], n[-1] = 0, (1 << 13) - 1
    cols["bitpacked13"] = (bytes([CM.BITPACKED]) + CM.stats_bytes(1 << 40, (1 << 40) + 1000 * 8191, 1000, rows) + _pack(n, 13),
                           np.uint64(1 << 40) + np.uint64(1000) * n)
    x = np.arange(rows, dtype=np.uint64)
    d = rng.integers(0, 64, size=rows).astype(np.uint64)
    v = np.uint64(1000) + x * np.uint64(9) + d  # (rows * 9 < 2^31: the product's bits 32..63 are the row times 9)
    assert rows * 9 < 1 << 31
    cols["linear6"] = (bytes([CM.LINEAR]) + CM.stats_bytes(int(v.min()), int(v.max()), 1, rows) + CM.vint(9 << 32) + CM.vint(1000) +
                       bytes([6]) + _pack(d, 6), v)
    d = rng.integers(0, 1 << 11, size=rows).astype(np.uint64)
    d[0] = 0
    blk = x // np.uint64(512)
    v = blk * np.uint64(21 * 512) + (x % np.uint64(512)) * np.uint64(21) + d
    n_blocks = (rows + 511) // 512
    footer = b"".join(CM.vint(21 << 32) + CM.vint(21 * 512 * b) + bytes([11]) for b in range(n_blocks))
    cols["blockwise11"] = (bytes([CM.BLOCKWISE]) + CM.stats_bytes(0, int(v.max()), 1, rows) + _pack(d, 11) + footer +
                           len(footer).to_bytes(4, "little"), v)
    for name, (blob, vals) in cols.items():
        for r in (0, 1, 511, 512, 513, rows // 2, rows - 1):
            assert CM.read_one(blob, r) == int(vals[r]), (name, r)
    return cols


def child(args):
    import ctypes as C

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from oracle import oracle as O
    from tests import column_model as CM
    import tantivy_amd as T

    B = T.binding
    seg = O.synth_segment(args.docs, n_terms=args.terms, with_positions=False)
    md = seg.max_doc
    dev = T.DeviceIndex([seg], devices=[0])
    dev.set_option("timing", 1)
    raw = dev.segment_raw(0)
    rng = np.random.default_rng(20261019)
    cols = make_columns(md, rng)
    present = rng.random(md) < 0.5
    n_present = int(present.sum())
    blob, vals = make_columns(n_present, rng)["bitpacked13"]
    uploads = {name: (dev.add_column(b), v, None) for name, (b, v) in cols.items()}
    uploads["bitpacked13_optional"] = (dev.add_column(blob, CM.OPTIONAL, CM.presence_words(present)), vals, present)
    # ---- builds
    build, handles = {}, {}
    for name, (col, vals, pres) in uploads.items():
        srt = np.sort(vals[:: max(1, vals.size // 100_000)])
        mid = int(srt[srt.size // 2])
        spans = {"narrow": (mid, int(srt[min(srt.size - 1, srt.size // 2 + srt.size // 1000)])),
                 "wide": (int(srt[srt.size // 4]), int(srt[3 * srt.size // 4]))}
        info = dev.column_info(col)
        for rname, (lo, hi) in spans.items():
            ev, wall = [], []
            h = None
            for i in range(args.warmup + args.reps):
                if h is not None:
                    dev.term_set_release(h)
                t0 = time.perf_counter()
                h, _ = dev.range_prepare(col, ("in", lo), ("in", hi), 1.0)
                dt = (time.perf_counter() - t0) * 1e3
                st = dev.last_batch_stats()
                if i >= args.warmup:
                    ev.append(st["kernel_ms"])
                    wall.append(dt)
            n_docs = dev.term_set_info(h)[0]
            assert n_docs == int(((vals >= np.uint64(lo)) & (vals <= np.uint64(hi))).sum()), (name, rname)
            med = float(np.median(ev))
            model = int(st["algorithmic_bytes"])
            gbs = model / (med * 1e-3) / 1e9
            build["%s/%s" % (name, rname)] = {
                "codec": info["codec"], "cardinality": info["cardinality"], "rows": info["num_rows"], "resident_bytes": info["resident_bytes"],
                "docs_in_range": int(n_docs), "build_kernel_ms": _stat(ev), "prepare_wall_ms": _stat(wall), "algorithmic_bytes": model,
                "implied_GBs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
            handles["%s/%s" % (name, rname)] = h
    # ---- `+a +range` batches
    n, k = args.queries, 10
    by_df = sorted(range(len(seg.terms)), key=lambda t: -seg.terms[t].doc_freq)
    terms = [by_df[i % len(by_df)] for i in range(n)]
    avg = seg.avg_fieldnorm
    w_of = {t: float(O.bm25_for_one_term(seg.terms[t].doc_freq, md, avg).weight) for t in set(terms)}
    cache = np.array(list(O.bm25_for_one_term(1, md, avg).cache), np.float32)
    batches = {}
    for key, h in handles.items():
        sq = [(T.MODE_AND, [a, h], None) for a in terms]
        fq = [(T.MODE_AND, [a, h]) for a in terms]
        ws = [[w_of[a], 1.0] for a in terms]
        ms = []
        for i in range(args.warmup + args.reps):
            dev.raw_search(sq, ws, cache, k)
            st = dev.last_batch_stats()
            if i >= args.warmup:
                ms.append(st["kernel_ms"])
        sizes = dev.last_batch_match_counts(n)
        qs, keep = dev._raw_scored_queries(fq, ws, cache, 0)  # marshalled once: the timed region is the C call alone
        counts = np.zeros(n, np.uint32)
        cw = []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            B._check(B.lib().tq_count_batch(raw, qs, n, B._u32(counts)))
            if i >= args.warmup:
                cw.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(counts, sizes), key
        batches[key] = {"queries": n, "k": k, "search_kernel_ms": _stat(ms), "search_kernels": st["kernels"],
                        "search_algorithmic_bytes": int(st["algorithmic_bytes"]), "count_wall_ms": _stat(cw),
                        "matches": int(sizes.astype(np.int64).sum())}
    print("RESULT " + json.dumps({
        "docs": md, "terms": args.terms, "reps": args.reps, "warmup": args.warmup, "hbm_peak_GBs": HBM_PEAK_GBS,
        "byte_model": "payload bytes + 16 B per 32 docs (table written, read once by the scan) + 8 B per 32 docs of presence table (Optional)",
        "note": "first measurement of this path: records, not pass bars", "build": build, "must_a_must_range": batches}))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--terms", type=int, default=256)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_bench.json"))
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
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"bench": "tools/bench_range.py", "device": "MI355X", "result": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
