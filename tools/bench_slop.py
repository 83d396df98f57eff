#!/usr/bin/env python
"""Sloppy phrases on the device (TQ_MODE_PHRASE with slop > 0: tq_phrase_slop.hip, TQ_KERNEL_PHRASE_SLOP) against the exact
phrase: bench.py's `phrase3` stream (three distinct ranks ~ Zipf(1) over the 64 most frequent terms of a 10 M-doc
segment with planted phrase positions, offsets = the rank differences) at slop 0, 1, 2 and 4, and its 2-term variant (the
first two terms of every query) at the same slops, k = 10, through tq_search_batch_opts.

slop 0 takes the exact-phrase kernels (phrase_kernel / phrase_sweep_kernel), which this route does not touch: that row IS
the parent commit's figure, measured in the same run on the same segment, and the cost of a slop is read against it.

Per run: q/s over the wall time of the C call (it ends in a synchronise), kernel ms per 1 000 queries (HIP events, option
"timing"), kernel_mask, the per-query overflow words (a non-zero word makes the call TQ_ERR_UNSUPPORTED: the run is still
timed, the number of such queries is recorded) and the share of queries with a list that holds a slot of the probe pool
after the runs (tq_term_table_info: the segment's own record).  algorithmic_bytes is the header's MODEL, not a measurement.

Protocol: `warmup` untimed runs (they also build the probe tables), then `reps` timed runs; median, minimum and maximum.
No target is set: nobody has measured this route before.  The parent starts one child process under a time limit; the
JSON goes to profiles/slop_bench.json.

  python tools/bench_slop.py [--docs 10000000] [--terms 256] [--queries 1000] [--reps 5] [--warmup 2]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SLOPS = (0, 1, 2, 4)
ERR_UNSUPPORTED = 4


def _stat(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(np.min(xs)), 4), "max": round(float(np.max(xs)), 4)}


def child(args):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    import bench
    from oracle import oracle as O
    import tantivy_amd as T

    B = T.binding
    seg = O.synth_segment(args.docs, n_terms=args.terms, with_positions=True, phrase_terms=bench.PHRASE_TERMS)
    dev = T.DeviceIndex([seg], devices=[0])
    dev.set_option("timing", 1)
    base, k = bench.build_queries(O, "phrase3", args.queries, None)
    streams = {"phrase3": [(q[1], q[2]) for q in base], "phrase2": [(q[1][:2], q[2][:2]) for q in base]}
    avg = seg.avg_fieldnorm
    cache = np.array(list(O.bm25_for_one_term(1, seg.max_doc, avg).cache), np.float32)
    out = {}
    for name, stream in streams.items():
        ws = [[float(O.bm25_for_terms([seg.terms[t].doc_freq for t in terms], seg.max_doc, avg).weight)] for terms, _ in stream]
        runs = {}
        for slop in SLOPS:
            queries = [(T.MODE_PHRASE, terms, offs, slop) for terms, offs in stream]
            wall, kern = [], []
            rc = 0
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                rc, _, _, counts = dev.raw_search_trees(queries, ws, cache, k, return_rc=True)
                dt = time.perf_counter() - t0
                if rc not in (0, ERR_UNSUPPORTED):
                    raise SystemExit("slop %d: rc %d: %s" % (slop, rc, B.lib().tq_last_error().decode()))
                st = dev.last_batch_stats()
                if i >= args.warmup:
                    wall.append(dt * 1e3)
                    kern.append(st["kernel_ms"])
            over = dev.last_batch_slop_overflows(len(queries))
            if rc == ERR_UNSUPPORTED and not int((over > 0).sum()):
                raise SystemExit("slop %d: refused: %s" % (slop, B.lib().tq_last_error().decode()))
            runs[str(slop)] = {
                "queries": len(queries), "k": k, "kernel_mask": int(st["kernel_mask"]), "kernels": st["kernels"],
                "wall_ms": _stat(wall), "qps": round(len(queries) / (float(np.median(wall)) * 1e-3), 1),
                "kernel_ms_per_1000_queries": _stat([x * 1000.0 / len(queries) for x in kern]),
                "overflow_queries": int((over > 0).sum()), "overflow_docs": int(over.astype(np.int64).sum()),
                "hits": int(counts.astype(np.int64).sum()), "algorithmic_bytes_model": int(st["algorithmic_bytes"]),
            }
        # after the sloppy runs: which lists hold a slot of the probe pool (tq_term_table_info), as the segment says
        slot_of = {t: dev.term_table_info(dev.term_handle(t))["probe_slot"] for terms, _ in stream for t in terms}
        probe = sum(any(slot_of[t] != 0xFFFFFFFF for t in terms) for terms, _ in stream)
        s0 = runs["0"]["kernel_ms_per_1000_queries"]["median"]
        out[name] = {"probe_pool_query_share": round(probe / len(stream), 4), "slop": runs,
                     "slop0_is": "the exact-phrase kernels of the parent commit (untouched by this route), same run, same segment",
                     "kernel_ms_ratio_to_slop0": {s: round(runs[s]["kernel_ms_per_1000_queries"]["median"] / s0, 2) if s0 else None
                                                  for s in runs}}
    print("RESULT " + json.dumps({"device": torch.cuda.get_device_name(0), "docs": args.docs, "terms": args.terms, "reps": args.reps, "warmup": args.warmup, "streams": out}))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--terms", type=int, default=256)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slop_bench.json"))
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
        json.dump({"bench": "tools/bench_slop.py", "device": res.pop("device"), "result": res}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
