#!/usr/bin/env python
"""Full doc sets on the device (tq_docset_batch_device) against the Count collector over the same bitmap words
(tq_count_batch with "count_bitmap_ratio" forced to always): a 10 M-doc Zipf segment from the oracle's generator,
batches of and2, or5 and flat boolean queries from O.zipf_queries, each sized so that its output stays under 4 GB.

Count reads every list's words once and writes nothing; the doc-set call reads them twice (count pass, write pass)
and writes 4 bytes per doc: the yardstick is 2 x the count time + docs x 4 B at the fill bandwidth of the same run.

The parent starts one fresh child process per workload, each under its own time limit, and stops at the first that
fails.  Per workload one JSON line; all of them go to profiles/docset_bench.json.

--scores: the same batches through tq_docset_scored_batch_device as well, alternating with the unscored call in one
process: the scored call's kernel time, the scoring pass as the difference of the two, what the byte model predicts
for the bytes the pass adds at the fill bandwidth of the same run, and — for context — the exhaustive top-10 search of the
same queries, the only route that scored every match before.  Written to profiles/docset_scored_bench.json.

--trees: doc sets of phrase and nested boolean queries (option "docset_trees", tq_docset_tree.hip) on the 10 M-doc
segment WITH positions that bench.py's phrase workloads build: `phrase2` (2-term phrases over the phrase terms) and
`nested` (the shapes of tests/tree_shapes.py::SHAPES over Zipf ids).  Per workload, from one process: the doc-set
call's kernel and batch ms, the docs written, and the ms of tq_count_batch for the same queries — the exhaustive
scan, the only device route that visited every match of these shapes before, and therefore the yardstick — plus the
fill of the output buffer, what a write of the same size costs at the least.  Written to
profiles/docset_tree_bench.json.

--trees --scores: the two batches of --trees through tq_docset_scored_batch_device (option "docset_score_trees",
tq_docset_tree_score.hip), alternating with the unscored call in one process, HIP events around all kernels of a call,
the median of --reps (default here: 10) warm repetitions: the unscored and the scored call, the scoring pass as their
difference, what the byte model predicts for the bytes the pass adds at the fill bandwidth of the same run, and the
exhaustive top-10 search of the same queries (tq_search_batch: the route that scored every match of these shapes
before, ten rows per query); a sample of rows is checked against the oracle in the same process.  Written to
profiles/docset_tree_scored_bench.json.

  python tools/bench_docset.py [--docs 10000000] [--reps 20] [--warmup 3] [--scores] [--trees]"""
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
WORKLOADS = ("and2", "or5", "bool")
TREE_WORKLOADS = ("phrase2", "nested")
PHRASE_TERMS = 64  # ranks with planted phrase positions, as in bench.py


def _queries(O, T, workload, n, terms):
    if workload == "and2":
        return [(O.MODE_AND, q.tolist()) for q in O.zipf_queries(n, 2, terms, seed=20260921)]
    if workload == "or5":
        return [(O.MODE_OR, q.tolist()) for q in O.zipf_queries(n, 5, terms, seed=20260922)]
    # the shapes of bench.py's "bool" workload (an m-of-n shape would be scanned by Count: no yardstick for it)
    M, S, N = T.MUST, T.SHOULD, T.MUST_NOT
    shapes = [(3, [M, M, M], [0, 1, 1]), (4, [M, M, M, M], [0, 0, 1, 1]), (3, [M, S, N], None), (3, [M, M, M], [0, 0, 1])]
    ids = O.zipf_queries(n, 4, terms, seed=20260924)
    return [(T.MODE_BOOL, q.tolist()[:shapes[i % 4][0]], shapes[i % 4][1], shapes[i % 4][2], 0) for i, q in enumerate(ids)]


def child(args):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from oracle import oracle as O
    import tantivy_amd as T

    seg = O.synth_segment(args.docs, n_terms=args.terms, with_positions=False)
    dev = T.DeviceIndex([seg], devices=[0])
    dev.set_option("timing", 1)
    dev.set_option("count_bitmap_ratio", 1 << 30)  # Count: always from bitmap words
    n = args.queries
    queries = _queries(O, T, args.child, n, args.terms)
    counts = dev.count(queries)
    while int(counts.sum()) * 4 > OUT_BYTES_MAX and n > 1:  # size the batch by its output
        n = max(1, int(n * OUT_BYTES_MAX / (int(counts.sum()) * 4) * 0.95))
        queries, counts = queries[:n], counts[:n]
    total = int(counts.sum())
    d_docs = torch.empty(max(1, total), dtype=torch.int32, device="cuda")
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()

    def docset_step():
        rc = dev.raw_docset_device(queries, d_docs, total, d_starts, stream=stream.cuda_stream)
        assert rc == 0, T.binding.lib().tq_last_error()

    ds_ms, ds_wall, ct_wall = [], [], []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        docset_step()
        st = dev.last_batch_stats()  # waits for the batch; kernel_ms = HIP events around scatter + count + scan + write
        wall = (time.perf_counter() - t0) * 1e3
        if i >= args.warmup:
            ds_ms.append(st["kernel_ms"])
            ds_wall.append(wall)
    assert st["kernels"] == ["docset"] and st["matches"] == total, st
    starts = d_starts.cpu().numpy()
    assert int(starts[-1]) == total and np.array_equal(np.diff(starts), counts.astype(np.int64))
    # a sample of rows against the oracle
    docs = None
    for q in range(0, n, max(1, n // 8)):
        if counts[q] > 2_000_000:
            continue
        if queries[q][0] == T.MODE_BOOL:
            w, _ = O.bool_match_all(seg, queries[q][1], queries[q][2], queries[q][3], queries[q][4])
        else:
            w, _ = O.match_all(seg, queries[q][1], queries[q][0])
        got = d_docs[int(starts[q]): int(starts[q + 1])].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, np.asarray(w, np.uint32)), queries[q]
    dev.prepare(queries)
    out = np.zeros(max(1, n), np.uint64)
    import ctypes as C
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        T.binding._check(T.binding.lib().tqh_count_prepared(dev._s, out.ctypes.data_as(C.POINTER(C.c_uint64))), host=True)
        if i >= args.warmup:
            ct_wall.append((time.perf_counter() - t0) * 1e3)
    assert dev.last_batch_stats()["kernels"] == ["count_bitmaps"]
    assert np.array_equal(out[:n], counts)
    # the fill bandwidth of this run: a device memset of the output buffer
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fill = []
    for i in range(args.warmup + args.reps):
        ev0.record()
        d_docs.fill_(i)
        ev1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            fill.append(ev0.elapsed_time(ev1))
    lists = st["algorithmic_bytes"] - 4 * total  # lists x bitmap words x 4
    scored = scored_run(args, O, T, seg, dev, queries, total, d_docs, d_starts, stream, float(np.median(fill))) if args.scores else {}
    k = float(np.median(ds_ms))
    res = {"workload": args.child, "docs": args.docs, "terms": args.terms, "queries": n, "out_docs": total,
           "docset_kernel_ms": round(k, 4), "docset_kernel_ms_min": round(float(np.min(ds_ms)), 4),
           "docset_wall_ms": round(float(np.median(ds_wall)), 4),
           "count_wall_ms": round(float(np.median(ct_wall)), 4),
           "fill_ms": round(float(np.median(fill)), 4),
           "fill_GBs": round(4 * total / (float(np.median(fill)) * 1e-3) / 1e9, 1) if total else None,
           "yardstick_ms": round(2 * float(np.median(ct_wall)) + float(np.median(fill)), 4),
           "algorithmic_bytes": int(st["algorithmic_bytes"]), "list_word_bytes": int(lists),
           "model_GBs": round(st["algorithmic_bytes"] / (k * 1e-3) / 1e9, 1),
           "model_frac_of_peak": round(st["algorithmic_bytes"] / (k * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "stage_min_docs": int(os.environ.get("TQ_DOCSET_STAGE_MIN", "2048")), "reps": args.reps, "warmup": args.warmup, "rows_checked_against_oracle": True}
    res.update(scored)
    print("RESULT " + json.dumps(res))
    dev.close()


def _tree_queries(O, T, workload, n, terms):
    """-> (device tuples, oracle forms)"""
    from tests.tree_shapes import SHAPES, to_device

    if workload == "phrase2":  # two distinct ranks in rank order, offsets = the rank difference (bench.py's phrase3, one term shorter)
        qs = []
        for q in O.zipf_queries(n, 2, PHRASE_TERMS, seed=20260925):
            r = sorted(int(x) for x in q)
            qs.append((O.MODE_PHRASE, r, [0, r[1] - r[0]]))
        return qs, [("phrase", q[1], q[2]) for q in qs]
    specs = [(SHAPES[i % len(SHAPES)][0](q.tolist()), SHAPES[i % len(SHAPES)][1])
             for i, q in enumerate(O.zipf_queries(n, 8, terms, seed=20260926))]
    return [to_device(T, sp, msm) for sp, msm in specs], [("tree", sp, msm) for sp, msm in specs]


def tree_child(args):
    import ctypes as C

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from oracle import oracle as O
    import tantivy_amd as T

    seg = O.synth_segment(args.docs, n_terms=args.terms, with_positions=True, phrase_terms=PHRASE_TERMS)
    dev = T.DeviceIndex([seg], devices=[0])
    dev.set_option("timing", 1)
    dev.set_option("docset_trees", 1)
    n = args.queries
    queries, forms = _tree_queries(O, T, args.child, n, args.terms)
    counts = dev.count(queries)  # (the scan; it also builds the probe tables both routes use)
    while int(counts.sum()) * 4 > OUT_BYTES_MAX and n > 1:  # size the batch by its output
        n = max(1, int(n * OUT_BYTES_MAX / (int(counts.sum()) * 4) * 0.95))
        queries, forms, counts = queries[:n], forms[:n], counts[:n]
    total = int(counts.sum())
    d_docs = torch.empty(max(1, total), dtype=torch.int32, device="cuda")
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    ds_ms, ds_wall, ct_wall, ct_kernel = [], [], [], []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        rc = dev.raw_docset_device(queries, d_docs, total, d_starts, stream=stream.cuda_stream)
        assert rc == 0, T.binding.lib().tq_last_error()
        st = dev.last_batch_stats()  # waits for the batch; kernel_ms = HIP events around bits + count + scan + write
        wall = (time.perf_counter() - t0) * 1e3
        if i >= args.warmup:
            ds_ms.append(st["kernel_ms"])
            ds_wall.append(wall)
    assert st["kernels"] == ["docset", "docset_tree"] and st["matches"] == total, st
    starts = d_starts.cpu().numpy()
    assert int(starts[-1]) == total and np.array_equal(np.diff(starts), counts.astype(np.int64))
    checked = 0
    for q in range(0, n, max(1, n // 6)):  # a sample of rows against the oracle
        if counts[q] > 2_000_000:
            continue
        f = forms[q]
        w = O.match_all(seg, f[1], O.MODE_PHRASE, phrase_offsets=f[2])[0] if f[0] == "phrase" else O.tree_match_all(seg, f[1], f[2])[0]
        got = d_docs[int(starts[q]): int(starts[q + 1])].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, np.asarray(w, np.uint32)), queries[q]
        checked += 1
    dev.prepare(queries)
    out = np.zeros(max(1, n), np.uint64)
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        T.binding._check(T.binding.lib().tqh_count_prepared(dev._s, out.ctypes.data_as(C.POINTER(C.c_uint64))), host=True)
        if i >= args.warmup:
            ct_wall.append((time.perf_counter() - t0) * 1e3)
            ct_kernel.append(dev.last_batch_stats()["kernel_ms"])
    scan = dev.last_batch_stats()
    assert np.array_equal(out[:n], counts)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fill = []
    for i in range(args.warmup + args.reps):  # the fill bandwidth of this run: a device memset of the output buffer
        ev0.record()
        d_docs.fill_(i)
        ev1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            fill.append(ev0.elapsed_time(ev1))
    k = float(np.median(ds_ms))
    res = {"workload": args.child, "docs": args.docs, "terms": args.terms, "queries": n, "out_docs": total,
           "docset_kernel_ms": round(k, 4), "docset_kernel_ms_min": round(float(np.min(ds_ms)), 4),
           "docset_batch_ms": round(float(np.median(ds_wall)), 4),
           "count_scan_ms": round(float(np.median(ct_wall)), 4), "count_scan_kernel_ms": round(float(np.median(ct_kernel)), 4),
           "count_scan_kernels": scan["kernels"],
           "fill_ms": round(float(np.median(fill)), 4),
           "scan_plus_fill_ms": round(float(np.median(ct_wall)) + float(np.median(fill)), 4),
           "algorithmic_bytes": int(st["algorithmic_bytes"]),
           "model_GBs": round(st["algorithmic_bytes"] / (k * 1e-3) / 1e9, 1),
           "reps": args.reps, "warmup": args.warmup, "rows_checked_against_oracle": checked}
    print("RESULT " + json.dumps(res))
    dev.close()


def tree_scored_child(args):
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from oracle import oracle as O
    import tantivy_amd as T

    seg = O.synth_segment(args.docs, n_terms=args.terms, with_positions=True, phrase_terms=PHRASE_TERMS)
    dev = T.DeviceIndex([seg], devices=[0])
    dev.set_option("timing", 1)
    dev.set_option("docset_trees", 1)
    dev.set_option("docset_score_trees", 1)
    n = args.queries
    queries, forms = _tree_queries(O, T, args.child, n, args.terms)
    counts = dev.count(queries)  # (it also builds the probe tables every route uses)
    while int(counts.sum()) * 8 > OUT_BYTES_MAX and n > 1:  # size the batch by its output: docs + scores
        n = max(1, int(n * OUT_BYTES_MAX / (int(counts.sum()) * 8) * 0.95))
        queries, forms, counts = queries[:n], forms[:n], counts[:n]
    total = int(counts.sum())
    # the oracle's weights: one Bm25Weight per term, one per phrase on each of its terms; the segment's cache
    avg = seg.avg_fieldnorm
    one = O.bm25_for_one_term(1, seg.max_doc, avg)
    cache = np.array(list(one.cache), np.float32)
    w_of = {}
    weights = []
    for q, f in zip(queries, forms):
        if f[0] == "phrase":
            weights.append([float(O.default_weights(seg, f[1], O.MODE_PHRASE)[0].weight)] * len(f[1]))
            continue
        for t in q[1]:
            if t not in w_of:
                w_of[t] = float(O.bm25_for_one_term(seg.terms[t].doc_freq, seg.max_doc, avg).weight)
        weights.append([w_of[t] for t in q[1]])
    d_docs = torch.empty(max(1, total), dtype=torch.int32, device="cuda")
    d_docs2 = torch.empty(max(1, total), dtype=torch.int32, device="cuda")
    d_scores = torch.empty(max(1, total), dtype=torch.float32, device="cuda")
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    plain_ms, scored_ms = [], []
    for i in range(args.warmup + args.reps):
        rc = dev.raw_docset_device(queries, d_docs2, total, d_starts, stream=stream.cuda_stream)
        assert rc == 0, T.binding.lib().tq_last_error()
        a = dev.last_batch_stats()  # waits for the batch; kernel_ms = HIP events around all kernels of the call
        rc = dev.raw_docset_scored_device(queries, d_docs, d_scores, total, d_starts, stream=stream.cuda_stream,
                                          weights=weights, cache=cache)
        assert rc == 0, T.binding.lib().tq_last_error()
        b = dev.last_batch_stats()
        if i >= args.warmup:
            plain_ms.append(a["kernel_ms"])
            scored_ms.append(b["kernel_ms"])
    assert a["kernels"] == ["docset", "docset_tree"] and a["matches"] == total, a
    assert b["kernels"] == ["docset", "docset_score", "docset_tree", "docset_tree_score"] and b["matches"] == total, b
    assert torch.equal(d_docs, d_docs2)  # the rows are the unscored call's
    starts = d_starts.cpu().numpy()
    assert int(starts[-1]) == total and np.array_equal(np.diff(starts), counts.astype(np.int64))
    checked = 0
    for q in range(0, n, max(1, n // 6)):  # a sample of rows against the oracle: a phrase bit-equal, a tree within 1e-5
        if counts[q] > 2_000_000:
            continue
        f = forms[q]
        if f[0] == "phrase":
            wd, ws = O.match_all(seg, f[1], O.MODE_PHRASE, phrase_offsets=f[2])
        else:
            wd, ws = O.tree_match_all(seg, f[1], f[2])
        got_d = d_docs[int(starts[q]): int(starts[q + 1])].cpu().numpy().view(np.uint32)
        got_s = d_scores[int(starts[q]): int(starts[q + 1])].cpu().numpy()
        ws = np.asarray(ws, np.float32)
        assert np.array_equal(got_d, np.asarray(wd, np.uint32)), queries[q]
        assert np.array_equal(got_s, ws) if f[0] == "phrase" else np.allclose(got_s, ws, rtol=1e-5, atol=0), queries[q]
        checked += 1
    ex_ms = []
    for i in range(1 + 3):  # the exhaustive top-10 search of the same queries
        dev.raw_search_trees(queries, weights, cache, 10, (1, 0))
        e = dev.last_batch_stats()
        if i >= 1:
            ex_ms.append(e["kernel_ms"])
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fill = []
    for i in range(args.warmup + args.reps):  # the fill bandwidth of this run: a device memset of the output buffer
        ev0.record()
        d_docs.fill_(i)
        ev1.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            fill.append(ev0.elapsed_time(ev1))
    p_ms, s_ms, fill_ms = float(np.median(plain_ms)), float(np.median(scored_ms)), float(np.median(fill))
    added = int(b["algorithmic_bytes"]) - int(a["algorithmic_bytes"])  # 5 B per doc + 8 B per scoring list per 32 docs
    fill_gbs = 4 * total / (fill_ms * 1e-3) / 1e9 if total else float("nan")
    res = {"workload": args.child, "docs": args.docs, "terms": args.terms, "queries": n, "out_docs": total,
           "unscored_kernel_ms": round(p_ms, 4), "scored_kernel_ms": round(s_ms, 4),
           "scored_kernel_ms_min": round(float(np.min(scored_ms)), 4),
           "score_pass_ms": round(s_ms - p_ms, 4),
           "fill_ms": round(fill_ms, 4), "fill_GBs": round(fill_gbs, 1),
           "unscored_algorithmic_bytes": int(a["algorithmic_bytes"]), "scored_algorithmic_bytes": int(b["algorithmic_bytes"]),
           "score_pass_added_bytes": added, "score_pass_model_ms_at_fill_bw": round(added / (fill_gbs * 1e9) * 1e3, 4),
           "exhaustive_top10_kernel_ms": round(float(np.median(ex_ms)), 4), "exhaustive_kernels": e["kernels"],
           "reps": args.reps, "warmup": args.warmup, "rows_checked_against_oracle": checked}
    print("RESULT " + json.dumps(res))
    dev.close()


def scored_run(args, O, T, seg, dev, queries, total, d_docs, d_starts, stream, fill_ms):
    """The batch through tq_docset_scored_batch_device, alternating with the unscored call; -> the extra result fields."""
    import torch

    n = len(queries)
    avg = seg.avg_fieldnorm
    w_of = {}
    for q in queries:
        for t in q[1]:
            if t not in w_of:
                w_of[t] = O.bm25_for_one_term(seg.terms[t].doc_freq, seg.max_doc, avg)
    weights = [[float(w_of[t].weight) for t in q[1]] for q in queries]
    cache = np.array(list(w_of[queries[0][1][0]].cache), np.float32)
    d_scores = torch.empty(max(1, total), dtype=torch.float32, device="cuda")
    d_docs2 = torch.empty(max(1, total), dtype=torch.int32, device="cuda")
    plain_ms, scored_ms = [], []
    for i in range(args.warmup + args.reps):
        rc = dev.raw_docset_device(queries, d_docs2, total, d_starts, stream=stream.cuda_stream)
        assert rc == 0, T.binding.lib().tq_last_error()
        a = dev.last_batch_stats()
        rc = dev.raw_docset_scored_device(queries, d_docs, d_scores, total, d_starts, stream=stream.cuda_stream,
                                          weights=weights, cache=cache)
        assert rc == 0, T.binding.lib().tq_last_error()
        b = dev.last_batch_stats()
        if i >= args.warmup:
            plain_ms.append(a["kernel_ms"])
            scored_ms.append(b["kernel_ms"])
    assert b["kernels"] == ["docset", "docset_score"] and b["matches"] == total, b
    assert torch.equal(d_docs, d_docs2)  # the rows are the unscored call's
    starts = d_starts.cpu().numpy()
    n_lists = []
    for q in range(0, n, max(1, n // 8)):  # a sample of rows against the oracle: bit-equal up to two lists, 1e-5 beyond
        if starts[q + 1] - starts[q] > 2_000_000:
            continue
        if queries[q][0] == T.MODE_BOOL:
            _, w = O.bool_match_all_c(seg, queries[q][1], queries[q][2], queries[q][3], queries[q][4])
            n_sc = sum(1 for o in queries[q][2] if o != T.MUST_NOT)
        else:
            _, w = O.match_all(seg, queries[q][1], queries[q][0])
            n_sc = len(queries[q][1])
        got = d_scores[int(starts[q]): int(starts[q + 1])].cpu().numpy()
        w = np.asarray(w, np.float32)
        assert got.shape == w.shape, queries[q]
        assert np.array_equal(got, w) if n_sc <= 2 else np.allclose(got, w, rtol=1e-5, atol=0), queries[q]
        n_lists.append(n_sc)
    # the exhaustive top-10 search of the same queries (tq_search_batch, option exhaustive for the call)
    sq = [(q[0], q[1], None) + ((q[2], q[3], q[4]) if q[0] == T.MODE_BOOL else ()) for q in queries]
    ex_ms = []
    for i in range(1 + 3):
        dev.raw_search(sq, weights, cache, 10, opts=(1, 0))
        e = dev.last_batch_stats()
        if i >= 1:
            ex_ms.append(e["kernel_ms"])
    p_ms, s_ms = float(np.median(plain_ms)), float(np.median(scored_ms))
    added = int(b["algorithmic_bytes"]) - int(a["algorithmic_bytes"])  # 5 B per doc + 8 B per scoring list per 32 docs
    fill_gbs = 4 * total / (fill_ms * 1e-3) / 1e9 if total else float("nan")
    return {"unscored_kernel_ms": round(p_ms, 4), "scored_kernel_ms": round(s_ms, 4),
            "scored_kernel_ms_min": round(float(np.min(scored_ms)), 4),
            "score_pass_ms": round(s_ms - p_ms, 4),
            "scored_algorithmic_bytes": int(b["algorithmic_bytes"]), "score_pass_added_bytes": added,
            "score_pass_model_ms_at_fill_bw": round(added / (fill_gbs * 1e9) * 1e3, 4),
            "scored_model_GBs": round(b["algorithmic_bytes"] / (s_ms * 1e-3) / 1e9, 1),
            "scored_model_frac_of_peak": round(b["algorithmic_bytes"] / (s_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "exhaustive_top10_kernel_ms": round(float(np.median(ex_ms)), 4), "exhaustive_kernels": e["kernels"],
            "scores_checked_against_oracle": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--terms", type=int, default=256)
    ap.add_argument("--queries", type=int, default=None, help="queries per batch (default: 1000; --trees: 512, one scratch bitmap each)")
    ap.add_argument("--reps", type=int, default=None, help="timed repetitions (default: 20; --trees --scores: 10)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--scores", action="store_true")
    ap.add_argument("--trees", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=WORKLOADS + TREE_WORKLOADS)
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 10 if args.scores and (args.trees or args.child in TREE_WORKLOADS) else 20
    if args.queries is None:
        args.queries = 512 if args.trees or args.child in TREE_WORKLOADS else 1000
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "docset_tree_scored_bench.json" if args.trees and args.scores else
                                "docset_tree_bench.json" if args.trees else
                                "docset_scored_bench.json" if args.scores else "docset_bench.json")
    if args.child in TREE_WORKLOADS:
        return tree_scored_child(args) if args.scores else tree_child(args)
    if args.child:
        return child(args)
    results = []
    for wl in (TREE_WORKLOADS if args.trees else WORKLOADS):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", wl, "--docs", str(args.docs), "--terms", str(args.terms),
               "--queries", str(args.queries), "--reps", str(args.reps), "--warmup", str(args.warmup)]
        if args.scores:
            cmd.append("--scores")
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit("%s: no result after %d s: stopping" % (wl, args.step_timeout))
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("%s failed (exit %d): stopping" % (wl, r.returncode))
        results.append(json.loads(line[-1][7:]))
        print(json.dumps(results[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"bench": "tools/bench_docset.py", "device": "MI355X", "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
