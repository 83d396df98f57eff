#!/usr/bin/env python
"""Term sets on the device (tq_term_set_prepare: tq_termset.hip; fuzzy / regex / TermSetQuery clauses as const-score
lists): one 10 M-doc Zipf segment from the oracle's generator.

  build     sets of 16, 256 and 4 096 members drawn across the doc-freq range: the HIP-event time of the build (option
            "timing": tq_term_set_prepare brackets the zeroing and its three stages and leaves the time, the HBM model's
            bytes and the number of members it OR-ed word-wise in tq_batch_stats — what the device held, not a guess) and
            the model's bytes — the scattered members' posting bytes + 4 B per 32 docs per bitmap member + 8 B per 32
            docs written and read once by the scan — over the median as a fraction of 8 TB/s; beside it the wall ms of
            the whole C call (uploads, launches, the blocking copy of the doc count)
  batches   1 000 queries with k = 10 of `set`, `+a +set`, `+a +b +set` and `a b set`, every query with one of 8 sets of 64
            members, through tq_search_batch (kernel ms from tq_last_batch_stats, option "timing"), tq_count_batch (wall
            ms of the C call: it ends in a synchronise) and tq_docset_scored_batch_device (kernel ms; the batch cut so
            that its rows stay under 4 GB)

Protocol: warm-up runs, then `reps` timed runs of every call; median, minimum and maximum.  Nothing could run these
shapes before: there is no threshold, this is the record.  The parent starts one child process under a time limit; the
JSON line goes to profiles/term_set_bench.json.

  python tools/bench_term_set.py [--docs 10000000] [--terms 8192] [--queries 1000] [--reps 10] [--warmup 2]"""
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
SET_SIZES = (16, 256, 4096)
SHAPES = ("set", "must_set", "must2_set", "should2_set")


def _stat(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(np.min(xs)), 4), "max": round(float(np.max(xs)), 4)}


def child(args):
    import ctypes as C

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from oracle import oracle as O
    import tantivy_amd as T

    B = T.binding
    M, S = T.MUST, T.SHOULD
    seg = O.synth_segment(args.docs, n_terms=args.terms, with_positions=False)
    dev = T.DeviceIndex([seg], devices=[0])
    dev.set_option("timing", 1)
    raw = dev.segment_raw(0)
    by_df = sorted(range(len(seg.terms)), key=lambda t: seg.terms[t].doc_freq)
    rng = np.random.default_rng(20261019)
    # ---- build
    build = {}
    for size in SET_SIZES:
        # across the doc-freq range: every (n_terms / size)-th term by doc freq
        members = [by_df[int(i)] for i in np.linspace(0, len(by_df) - 1, size).astype(int)]
        hs = np.array([dev.term_handle(t) for t in members], np.uint32)  # (prepares the members: not timed)
        out = C.c_uint32()
        ms, ev = [], []
        n_docs = model = n_bitmap = 0
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            B._check(B.lib().tq_term_set_prepare(raw, B._u32(hs), int(hs.size), C.byref(out)))
            dt = (time.perf_counter() - t0) * 1e3
            st = dev.last_batch_stats()  # the build's own figures (include/tantivy_amd.h, "term sets")
            model, n_bitmap = int(st["algorithmic_bytes"]), int(st["chunks"])
            n_docs = dev.term_set_info(out.value)[0]
            dev.term_set_release(out.value)
            if i >= args.warmup:
                ms.append(dt)
                ev.append(st["kernel_ms"])
        med = float(np.median(ev))
        build[str(size)] = {"members": size, "bitmap_members": n_bitmap, "docs": int(n_docs), "build_event_ms": _stat(ev),
                            "prepare_wall_ms": _stat(ms), "model_bytes": model,
                            "model_frac_of_peak": round(model / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    # ---- batches
    n, k = args.queries, 10
    sets = [dev.term_set_prepare([int(t) for t in rng.choice(len(seg.terms), size=64, replace=False)]) for _ in range(8)]
    pairs = [q.tolist() for q in O.zipf_queries(n, 2, min(256, args.terms), seed=20261019)]
    avg = seg.avg_fieldnorm
    w_of = {t: float(O.bm25_for_one_term(seg.terms[t].doc_freq, seg.max_doc, avg).weight) for p in pairs for t in p}
    cache = np.array(list(O.bm25_for_one_term(1, seg.max_doc, avg).cache), np.float32)
    sh = lambda i: sets[i % len(sets)]  # noqa: E731
    shapes = {  # (search tuple, flat tuple, weights)
        "set": [((T.MODE_OR, [sh(i)], None), (T.MODE_OR, [sh(i)]), [1.0]) for i in range(n)],
        "must_set": [((T.MODE_AND, [a, sh(i)], None), (T.MODE_AND, [a, sh(i)]), [w_of[a], 1.0]) for i, (a, _) in enumerate(pairs)],
        "must2_set": [((T.MODE_AND, [a, b, sh(i)], None), (T.MODE_AND, [a, b, sh(i)]), [w_of[a], w_of[b], 1.0])
                      for i, (a, b) in enumerate(pairs)],
        "should2_set": [((T.MODE_OR, [a, b, sh(i)], None), (T.MODE_OR, [a, b, sh(i)]), [w_of[a], w_of[b], 1.0])
                        for i, (a, b) in enumerate(pairs)],
    }
    stream = torch.cuda.Stream()
    results = {}
    for name in SHAPES:
        sq = [x[0] for x in shapes[name]]
        fq = [x[1] for x in shapes[name]]
        ws = [x[2] for x in shapes[name]]
        ms = []
        for i in range(args.warmup + args.reps):
            dev.raw_search(sq, ws, cache, k)
            st = dev.last_batch_stats()
            if i >= args.warmup:
                ms.append(st["kernel_ms"])
        assert st["kernels"] == ["tree"], st
        sizes = dev.last_batch_match_counts(n)
        cw = []
        qs, keep = dev._raw_scored_queries(fq, ws, cache, 0)  # marshalled once: the timed region is the C call alone
        counts = np.zeros(n, np.uint32)
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            B._check(B.lib().tq_count_batch(raw, qs, n, B._u32(counts)))
            if i >= args.warmup:
                cw.append((time.perf_counter() - t0) * 1e3)
        count_kernels = dev.last_batch_stats()["kernels"]
        assert np.array_equal(counts, sizes), name  # the doc set's size: what the unpruned search reports
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
            "search_model_frac_of_peak": round(st["algorithmic_bytes"] / (med * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "docs_in_sets": int(sizes.astype(np.int64).sum()), "count_wall_ms": _stat(cw), "count_kernels": count_kernels,
            "docset_scored_queries": n_ds, "docset_scored_docs": total, "docset_scored_kernel_ms": _stat(ds),
            "docset_scored_algorithmic_bytes": int(dst["algorithmic_bytes"]),
        }
    print("RESULT " + json.dumps({"docs": args.docs, "terms": args.terms, "reps": args.reps, "warmup": args.warmup,
                                  "hbm_peak_GBs": HBM_PEAK_GBS, "build": build, "shapes": results}))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--terms", type=int, default=8192)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "term_set_bench.json"))
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
        json.dump({"bench": "tools/bench_term_set.py", "device": "MI355X", "result": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
