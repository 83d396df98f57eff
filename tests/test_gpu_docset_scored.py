"""GPU parity of scored doc sets (tantivy_amd/csrc/tq_docset_score.hip; Weight::for_each -> for_each_scorer under
default_collect_segment_impl: src/query/weight.rs:9-18,89-97, src/collector/mod.rs:186-221): every alive matching doc
of a query, ascending, with its BM25 score in the unpruned scorers' summation order — the oracle's match_all.

Comparison rule (BASELINE.json, DESIGN.md "Exactness"): doc ids exact; scores bit-equal for queries with at most two
scoring lists, within 1e-5 relative otherwise.  Covers the tile / word / segment-tail boundaries, saturated tf bytes and
directory entries, every flat boolean shape (with the Should lists beside a Must part that the unscored descriptor
drops), the three access paths (bitmap, range directory, block search), the record options, the capacity protocol,
sub-batching, the refusals, the device-output variant and the multi-segment host mirror."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_docset import (BOUNDARY_MAX_DOC, ERR_INVALID, ERR_UNSUPPORTED, GUARD, _random_queries, _synth,
                                   _want)
from tests.test_gpu_round3 import _alive_bytes

pytestmark = pytest.mark.gpu

M, S, N = O.MUST, O.SHOULD, O.MUST_NOT
# Should lists beside a Must part with min_should_match == 0: they do not change the doc set, only the score
SHOULD_BESIDE_MUST = [([M, S, S], None, 0), ([M, M, S, S], None, 0), ([M, S, S, M, S], [0, 1, 1, 2, 3], 0)]


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


def _err(ta):
    return ta.binding.lib().tq_last_error()


def _guard_f32(a):
    return a.view(np.uint32)


def _weights(seg, queries, totals=None):
    """Per query the term weights the oracle uses (default_weights / bool_spec: one Bm25Weight per term; an absent term's
    weight is never read) and the Bm25Weight cache they share.  totals = (num_docs, num_tokens, doc freq per term id):
    index-wide statistics instead of the segment's."""
    nd, nt, dfs = totals if totals else (seg.max_doc, seg.total_num_tokens, None)
    avg = float(np.float32(nt) / np.float32(nd))
    out = []
    for q in queries:
        out.append([float(O.bm25_for_one_term(dfs[t] if dfs else seg.terms[t].doc_freq, nd, avg).weight)
                    if t < len(seg.terms) else 1.0 for t in q[1]])
    cache = np.array(list(O.bm25_for_one_term(1, nd, avg).cache), np.float32)
    return out, cache


def _n_scoring_lists(seg, q):
    occ = q[2] if q[0] == O.MODE_BOOL else [M] * len(q[1])
    return sum(1 for t, o in zip(q[1], occ) if o != N and t < len(seg.terms))


def _ref(seg, q, deleted=(), totals=None):
    """The oracle's ascending (docs, scores) of one query, deleted docs removed."""
    if q[0] == O.MODE_BOOL:
        cof, msm = (q[3] if len(q) > 3 else None), (q[4] if len(q) > 4 else 0)
        if totals:
            nd, nt, dfs = totals
            spec = O.bool_spec(seg, q[1], q[2], cof, msm, total_num_docs=nd, total_num_tokens=nt, dfs=[dfs[t] for t in q[1]])
            docs = np.zeros(max(1, seg.max_doc), np.uint32)
            scores = np.zeros(max(1, seg.max_doc), np.float32)
            n = O.lib().to_match_all(C.byref(seg.view), C.byref(spec.q), docs.ctypes.data_as(C.POINTER(C.c_uint32)),
                                     scores.ctypes.data_as(C.POINTER(C.c_float)), docs.size)
            d, s = docs[:n], scores[:n]
        else:
            d, s = O.bool_match_all_c(seg, q[1], q[2], cof, msm)
    else:
        w = None
        if totals:
            nd, nt, dfs = totals
            w = O.default_weights(seg, q[1], q[0], total_num_docs=nd, total_num_tokens=nt, dfs=[dfs[t] for t in q[1]])
        d, s = O.match_all(seg, q[1], q[0], weights=w)
    d, s = np.asarray(d, np.uint32), np.asarray(s, np.float32)
    if len(deleted):
        keep = ~np.isin(d, np.fromiter(deleted, np.uint32, len(deleted)))
        d, s = d[keep], s[keep]
    return d, s


def _assert_scored(seg, queries, docs, scores, starts, want, exact=False):
    """want = [(docs, scores)]; exact: bit equality whatever the number of lists."""
    assert len(starts) == len(queries) + 1
    for i, (q, (wd, ws)) in enumerate(zip(queries, want)):
        gd, gs = docs[int(starts[i]): int(starts[i + 1])], scores[int(starts[i]): int(starts[i + 1])]
        assert gd.size == wd.size and np.array_equal(gd, wd), (i, q, gd[:8], wd[:8], gd.size, wd.size)
        if exact or _n_scoring_lists(seg, q) <= 2:
            same = gs.view(np.uint32) == ws.view(np.uint32)
            assert np.all(same), (i, q, gd[~same][:4], gs[~same][:4], ws[~same][:4])
        else:
            assert np.allclose(gs, ws, rtol=1e-5, atol=0), (i, q, float(np.max(np.abs(gs - ws) / ws)))


# ---- 1. boundaries: hand-made lists around the word, tile and segment ends, tfs and fieldnorms that vary with the doc
@functools.lru_cache(maxsize=None)
def _boundary_segment():
    md = BOUNDARY_MAX_DOC
    a = [31, 32, 33, 63, 64, 65535, 65536, 65537, 131071, 131072, md - 1]
    lists = [a, list(range(md)), list(range(0, md, 2)), list(range(65530, 65545))]
    return O.build_segment(md, [[(d, 1 + d % 5) for d in l] for l in lists], [1 + d % 37 for d in range(md)]), a


@pytest.mark.parametrize("dense_ratio", [1 << 16, 4096, 2])
def test_scores_at_word_tile_and_segment_boundaries(ta, dense_ratio):
    """At 65 536 every list answers through its bitmap; at 4096 and at 2 the short lists A and D (below the range
    directories' minimum length) are searched block by block."""
    seg, a_docs = _boundary_segment()
    A, B, Cc, D, ABSENT = 0, 1, 2, 3, 77
    queries = [(O.MODE_OR, [B]), (O.MODE_AND, [A, B]), (ta.MODE_BOOL, [Cc], [N]), (ta.MODE_BOOL, [B, Cc], [M, N]),
               (O.MODE_AND, [A, ABSENT]), (ta.MODE_BOOL, [A, D, Cc], [S, S, N]), (O.MODE_OR, [A, ABSENT]), (O.MODE_OR, [D])]
    empty = (np.zeros(0, np.uint32), np.zeros(0, np.float32))
    want = [_ref(seg, queries[0]), _ref(seg, queries[1]), empty, _ref(seg, queries[3]), empty, _ref(seg, queries[5]),
            _ref(seg, (O.MODE_OR, [A])), _ref(seg, queries[7])]
    assert want[1][0].tolist() == a_docs and want[6][0].tolist() == a_docs
    assert want[3][0].size == 65_556 and np.unique(want[0][1]).size > 100
    weights, cache = _weights(seg, queries)
    total = sum(w[0].size for w in want)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", dense_ratio)
        dev.set_option("dense_budget_x", 256)
        rc, docs, scores, starts = dev.raw_docset_scored(queries, total, guard=8, weights=weights, cache=cache)
        assert rc == 0, _err(ta)
        assert int(starts[0]) == 0 and int(starts[-1]) == total
        _assert_scored(seg, queries, docs, scores, starts, want, exact=True)
        assert starts[2] == starts[3] and starts[4] == starts[5]  # empty rows between non-empty ones
        assert np.all(docs[total:] == GUARD) and np.all(_guard_f32(scores[total:]) == GUARD)
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == ta.binding.KERNEL_DOCSET | ta.binding.KERNEL_DOCSET_SCORE and st["matches"] == total, st
        n_in_place = sum(1 for t in seg.terms[:4] if t.doc_freq * dense_ratio >= seg.max_doc)
        assert n_in_place == (4 if dense_ratio == 1 << 16 else 2)
        assert dev.segment_stats(0)["n_dense_lists"] == n_in_place
        rc, docs_u, starts_u = dev.raw_docset(queries, total)  # the rows are the unscored call's
        assert rc == 0, _err(ta)
        assert np.array_equal(docs_u, docs[:total]) and np.array_equal(starts_u, starts)
    finally:
        dev.close()


# ---- 2. tf saturation: 255 in a tf byte, 0xFFFF in a range-directory entry
SAT_DOCS = [10, 31, 32, 63, 64, 4095, 4096, 65535, 65536]
SAT_TFS = [1, 254, 255, 256, 257, 65534, 65535, 65536, 70000]


@functools.lru_cache(maxsize=None)
def _saturation_segment(filler):
    """A = nine postings around the saturation points of the tf byte (255) and of the range-directory entry (0xFFFF);
    filler > 0: A also holds every `filler`-th odd doc above 1000 with tf 2, so that it is long enough for a range directory."""
    md = 70_000
    a = dict(zip(SAT_DOCS, SAT_TFS))
    if filler:
        a.update({d: 2 for d in range(1001, md, 2 * filler)})
    fn = [3] * md
    for d in SAT_DOCS:
        fn[d] = 1_000_000
    lists = [sorted(a.items()), [(d, 1 + d % 3) for d in range(0, md, 2)], [(d, 1) for d in range(md)]]
    return O.build_segment(md, lists, fn)


@pytest.mark.parametrize("structure", ["bitmap", "blocks", "rdir"])
def test_saturated_tfs_read_the_packed_value(ta, structure):
    """The nine scores of A are pairwise distinct f32 values whose neighbours around tf 65 535 differ by ~1.4e-6
    relative — below the tolerance of 3+ lists, so: 1- and 2-list queries only, bit-equal.  A behind a bitmap, searched
    block by block (nine postings are below the directories' minimum of 256), and — lengthened by filler postings — behind a
    range directory."""
    seg = _saturation_segment(40 if structure == "rdir" else 0)
    A, B, Cc = 0, 1, 2
    a_alone = _ref(seg, (O.MODE_OR, [A]))
    sat = np.isin(a_alone[0], SAT_DOCS)
    assert a_alone[0][sat].tolist() == SAT_DOCS and np.unique(a_alone[1][sat].view(np.uint32)).size == 9
    queries = [(O.MODE_OR, [A]), (O.MODE_AND, [A, B]), (O.MODE_AND, [A, Cc]), (O.MODE_OR, [A, B])]
    want = [_ref(seg, q) for q in queries]
    weights, cache = _weights(seg, queries)
    total = sum(w[0].size for w in want)
    tables = {}
    for budget in ([4] if structure == "bitmap" else [0, 4]):  # ("rdir_budget_x": without / with range directories)
        dev = ta.DeviceIndex([seg])
        try:
            dev.set_option("dense_ratio", 1 << 16 if structure == "bitmap" else 2)
            dev.set_option("dense_budget_x", 256)
            dev.set_option("rdir_budget_x", budget)
            rc, docs, scores, starts = dev.raw_docset_scored(queries, total, guard=4, weights=weights, cache=cache)
            assert rc == 0, _err(ta)
            _assert_scored(seg, queries, docs, scores, starts, want, exact=True)
            assert np.all(docs[total:] == GUARD) and np.all(_guard_f32(scores[total:]) == GUARD)
            stats = dev.segment_stats(0)
            tables[budget] = stats["term_table_bytes"]
            # which structure A got: a bitmap of its own, or none (B and C always have one)
            assert stats["n_dense_lists"] == (3 if structure == "bitmap" else 2)
        finally:
            dev.close()
    if structure == "rdir":    # ... and a range directory where it is long enough: one u32 per posting + the directory
        assert tables[4] - tables[0] >= 4 * seg.terms[A].doc_freq
    elif structure == "blocks":
        assert tables[4] == tables[0]


# ---- 3. random parity: every flat shape, the three access paths, with and without deletes
def _scored_queries(ta, rng, n_terms):
    queries = _random_queries(ta, rng, n_terms)
    for occ, cof, msm in SHOULD_BESIDE_MUST:
        terms = rng.choice(n_terms, size=len(occ), replace=False).tolist()
        queries.append((ta.MODE_BOOL, terms, list(occ), cof, msm))
    return queries


@pytest.mark.parametrize("seed", [31, 32])
@pytest.mark.parametrize("dense_ratio", [4096, 8])
def test_scored_docsets_equal_the_oracle(ta, seed, dense_ratio):
    rng = np.random.default_rng(seed)
    seg = _synth(100_000 + 999 * seed, 48)
    queries = _scored_queries(ta, rng, 48)
    deleted = rng.choice(seg.max_doc, size=seg.max_doc // 7, replace=False).tolist()
    weights, cache = _weights(seg, queries)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", dense_ratio)
        dev.set_option("dense_budget_x", 256)
        if seed == 32:
            dev.set_option("rdir_budget_x", 0)  # the lists without a bitmap: searched block by block
        for dels in ((), deleted):
            dev.set_alive_bitset(_alive_bytes(seg.max_doc, dels) if dels else None)
            want = [_ref(seg, q, dels) for q in queries]
            for q, w in zip(queries, want):
                assert np.array_equal(w[0], _want(seg, q, dels)), q  # (the two oracles agree on the doc sets)
            total = sum(w[0].size for w in want)
            rc, docs, scores, starts = dev.raw_docset_scored(queries, total, weights=weights, cache=cache)
            assert rc == 0, _err(ta)
            st = dev.last_batch_stats()
            assert st["kernel_mask"] == ta.binding.KERNEL_DOCSET | ta.binding.KERNEL_DOCSET_SCORE, st
            _assert_scored(seg, queries, docs, scores, starts, want)
            assert st["matches"] == total
            assert dev.last_batch_match_counts(len(queries)).tolist() == [w[0].size for w in want]
        used = {t for q in queries for t in q[1]}  # which of them have a bitmap: all at 4096, some at 8
        n_in_place = sum(1 for t in used if seg.terms[t].doc_freq * dense_ratio >= seg.max_doc)
        assert dev.segment_stats(0)["n_dense_lists"] == n_in_place
        assert n_in_place == len(used) if dense_ratio == 4096 else 0 < n_in_place < len(used) - 8
    finally:
        dev.close()


# ---- 4. record options
@pytest.mark.parametrize("option", ["basic", "no_fieldnorms"])
@pytest.mark.parametrize("dense_ratio", [4096, 2])
def test_record_options(ta, option, dense_ratio):
    """A TQ_BASIC segment (every tf reads as 1) and a segment without fieldnorms (the constant fieldnorm id)."""
    md = 70_001
    rng = np.random.default_rng(4)
    lists = [np.sort(rng.choice(md, size=n, replace=False)).tolist() for n in (30_000, 9_000, 700, 40)]
    if option == "basic":
        seg = O.build_segment(md, [[(d, 1) for d in l] for l in lists], [1 + d % 29 for d in range(md)], record_option=O.BASIC)
    else:
        seg = O.build_segment(md, [[(d, 1 + d % 7) for d in l] for l in lists], None, total_num_tokens=5 * md)
        assert seg.fieldnorm is None
    queries = [(O.MODE_AND, [0, 1]), (O.MODE_AND, [2, 0]), (O.MODE_OR, [1, 2, 3]), (O.MODE_OR, [0, 3, 2])]
    want = [_ref(seg, q) for q in queries]
    assert all(w[0].size for w in want) and all(np.all(np.isfinite(w[1])) and np.all(w[1] > 0) for w in want)
    weights, cache = _weights(seg, queries)
    total = sum(w[0].size for w in want)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", dense_ratio)
        dev.set_option("dense_budget_x", 256)
        rc, docs, scores, starts = dev.raw_docset_scored(queries, total, guard=4, weights=weights, cache=cache)
        assert rc == 0, _err(ta)
        _assert_scored(seg, queries, docs, scores, starts, want)
        assert np.all(_guard_f32(scores[total:]) == GUARD)
    finally:
        dev.close()


# ---- 5. capacity protocol
def test_capacity_protocol(ta):
    rng = np.random.default_rng(5)
    seg = _synth(100_000 + 999 * 31, 48)
    queries = _scored_queries(ta, rng, 48)[:24]
    want = [_ref(seg, q) for q in queries]
    weights, cache = _weights(seg, queries)
    total = sum(w[0].size for w in want)
    assert total > 1000
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 4096)
        dev.set_option("dense_budget_x", 256)
        rc, docs, scores, starts = dev.raw_docset_scored(queries, total, guard=64, weights=weights, cache=cache)
        assert rc == 0, _err(ta)
        _assert_scored(seg, queries, docs, scores, starts, want)
        assert np.all(docs[total:] == GUARD) and np.all(_guard_f32(scores[total:]) == GUARD)
        for cap in (total - 1, 0):
            rc2, docs2, scores2, starts2 = dev.raw_docset_scored(queries, cap, guard=total + 64 - cap, weights=weights,
                                                                 cache=cache)
            assert rc2 == ERR_INVALID
            assert _err(ta)
            assert np.array_equal(starts2, starts)  # complete: the caller sizes its retry from starts[n]
            assert np.all(docs2 == GUARD) and np.all(_guard_f32(scores2) == GUARD)  # no doc and no score at all
            rc3, docs3, scores3, starts3 = dev.raw_docset_scored(queries, int(starts2[-1]), weights=weights, cache=cache)
            assert rc3 == 0 and np.array_equal(starts3, starts)
            assert np.array_equal(docs3, docs[:total]) and np.array_equal(_guard_f32(scores3), _guard_f32(scores[:total]))
    finally:
        dev.close()


# ---- 6. sub-batching: the scoring pass follows every sub-batch's write pass
def test_sub_batches_score_their_own_rows(ta):
    seg = _synth(90_000, 64)
    queries = [(O.MODE_OR, [4 + i % 60, 4 + (i + 30) % 60]) for i in range(60)]
    sparse = {t for q in queries for t in q[1] if seg.terms[t].doc_freq * 8 < seg.max_doc}
    assert len(sparse) >= 40, len(sparse)
    want = [_ref(seg, q) for q in queries]
    weights, cache = _weights(seg, queries)
    total = sum(w[0].size for w in want)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 8)
        dev.set_option("docset_temp_lists", 16)
        rc, docs_s, scores_s, starts_s = dev.raw_docset_scored(queries, total, guard=16, weights=weights, cache=cache)
        assert rc == 0, _err(ta)
        dev.set_option("docset_temp_lists", 0)
        rc, docs_d, scores_d, starts_d = dev.raw_docset_scored(queries, total, weights=weights, cache=cache)
        assert rc == 0, _err(ta)
        _assert_scored(seg, queries, docs_s, scores_s, starts_s, want, exact=True)
        assert np.array_equal(starts_s, starts_d) and np.array_equal(docs_s[:total], docs_d)
        assert np.array_equal(_guard_f32(scores_s[:total]), _guard_f32(scores_d))
        assert np.all(docs_s[total:] == GUARD) and np.all(_guard_f32(scores_s[total:]) == GUARD)
        assert dev.last_batch_match_counts(len(queries)).tolist() == [w[0].size for w in want]
        assert dev.last_batch_stats()["matches"] == total
    finally:
        dev.close()


# ---- 7. refusals: the batch fails as a whole, names the query, and the segment stays usable
def test_refusals_leave_the_segment_usable(ta):
    seg = _synth(60_000, 48, with_positions=True)
    good = [(O.MODE_AND, [0, 1]), (O.MODE_OR, [2, 40])]
    want = [_ref(seg, q) for q in good]
    total = sum(w[0].size for w in want)
    phrase = (O.MODE_PHRASE, [0, 1], [0, 1])
    nested = (ta.MODE_BOOL, [1, 2, 3], [M, M, M], [0, 1, 1], 0, {"nested_occurs": [M, M, N]})
    bad_occur = (ta.MODE_BOOL, [1, 2], [M, 3])
    no_weights = (O.MODE_OR, [5, 6])
    dev = ta.DeviceIndex([seg])
    try:
        for bad, code in ((phrase, ERR_UNSUPPORTED), (nested, ERR_UNSUPPORTED), (bad_occur, ERR_INVALID),
                          (no_weights, ERR_INVALID)):
            for at in (0, 2):  # first and last of the batch
                batch = good[:at] + [bad] + good[at:]
                weights, cache = _weights(seg, batch)
                if bad is no_weights:
                    weights[at] = None
                rc, docs, scores, _ = dev.raw_docset_scored(batch, total + 1000, guard=4, weights=weights, cache=cache)
                assert rc == code, (bad, rc, _err(ta))
                assert ("query %d" % at).encode() in _err(ta), _err(ta)
                assert np.all(docs == GUARD) and np.all(_guard_f32(scores) == GUARD)  # nothing was launched
                weights, cache = _weights(seg, good)
                rc, docs, scores, starts = dev.raw_docset_scored(good, total, weights=weights, cache=cache)
                assert rc == 0, _err(ta)
                _assert_scored(seg, good, docs, scores, starts, want)
    finally:
        dev.close()


# ---- 8. device outputs
def test_device_variant(ta):
    import torch

    rng = np.random.default_rng(9)
    seg = _synth(100_000 + 999 * 32, 48)
    queries = _scored_queries(ta, rng, 48)[10:40]
    deleted = rng.choice(seg.max_doc, size=seg.max_doc // 7, replace=False).tolist()
    want = [_ref(seg, q, deleted) for q in queries]
    weights, cache = _weights(seg, queries)
    flat = np.concatenate([w[0] for w in want])
    total, n = flat.size, len(queries)
    want_starts = np.concatenate([[0], np.cumsum([w[0].size for w in want])]).astype(np.int64)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 8)
        dev.set_alive_bitset(_alive_bytes(seg.max_doc, deleted))
        guard32 = np.array([GUARD], np.uint32).view(np.int32)[0]
        for cap in (total // 2, total):
            dev.set_option("docset_temp_lists", 0 if cap < total else 16)  # (the full run: in sub-batches)
            d_docs = torch.full((total + 64,), int(guard32), dtype=torch.int32, device="cuda")
            d_scores = torch.full((total + 64,), int(guard32), dtype=torch.int32, device="cuda").view(torch.float32)
            d_starts = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            rc = dev.raw_docset_scored_device(queries, d_docs, d_scores, cap, d_starts, weights=weights, cache=cache)
            assert rc == 0, _err(ta)
            st = dev.last_batch_stats()  # (waits for the batch)
            torch.cuda.synchronize()
            docs = d_docs.cpu().numpy().view(np.uint32)
            scores = d_scores.cpu().numpy()
            starts = d_starts.cpu().numpy()
            assert np.array_equal(starts, want_starts)  # the full total, whatever the capacity
            assert np.all(docs[cap:] == GUARD) and np.all(_guard_f32(scores[cap:]) == GUARD)
            # below cap: whole rows, and the head of the row the capacity cuts
            cut = [(w[0][: max(0, cap - int(s0))], w[1][: max(0, cap - int(s0))]) for w, s0 in zip(want, want_starts)]
            _assert_scored(seg, queries, docs, scores, np.minimum(want_starts, cap), cut)
            assert st["kernel_mask"] == ta.binding.KERNEL_DOCSET | ta.binding.KERNEL_DOCSET_SCORE, st
            assert st["matches"] == total, st
    finally:
        dev.close()


# ---- 9. host mirror over two segments: scores under the index-wide statistics
def test_host_mirror_over_two_segments(ta):
    rng = np.random.default_rng(13)
    segs = [_synth(70_000, 48, 0), _synth(83_001, 48, 1)]
    queries = _scored_queries(ta, rng, 48)
    deleted = rng.choice(segs[1].max_doc, size=segs[1].max_doc // 5, replace=False).tolist()
    totals = (sum(s.max_doc for s in segs), sum(s.total_num_tokens for s in segs),
              [sum(s.terms[t].doc_freq for s in segs) for t in range(48)])
    dev = ta.DeviceIndex(segs)
    try:
        dev.set_option("dense_ratio", 8)
        dev.set_alive_bitset(_alive_bytes(segs[1].max_doc, deleted), segment_ord=1)
        got = dev.docset_scored(queries)
        plain = dev.docset(queries)
        for q, (g, gs), pl in zip(queries, got, plain):
            (d0, s0), (d1, s1) = _ref(segs[0], q, totals=totals), _ref(segs[1], q, deleted, totals=totals)
            want = np.concatenate([np.stack([np.zeros_like(d0), d0], axis=1), np.stack([np.ones_like(d1), d1], axis=1)])
            assert g.dtype == np.uint32 and g.shape == want.shape and np.array_equal(g, want), q
            assert np.array_equal(g, pl), q
            assert gs.dtype == np.float32 and gs.shape == (want.shape[0],)
            ws = np.concatenate([s0, s1])
            if _n_scoring_lists(segs[0], q) <= 2:
                assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), q
            else:
                assert np.allclose(gs, ws, rtol=1e-5, atol=0), q
    finally:
        dev.close()


# ---- 10. the unscored call is what it was
def test_unscored_call_unchanged(ta):
    rng = np.random.default_rng(31)
    seg = _synth(100_000 + 999 * 31, 48)
    queries = _scored_queries(ta, rng, 48)
    weights, cache = _weights(seg, queries)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 8)
        rc, docs0, starts0 = dev.raw_docset(queries, seg.max_doc * len(queries) // 4)
        assert rc == 0, _err(ta)
        total = int(starts0[-1])
        assert dev.last_batch_stats()["kernel_mask"] == ta.binding.KERNEL_DOCSET
        rc, docs_s, _, starts_s = dev.raw_docset_scored(queries, total, weights=weights, cache=cache)
        assert rc == 0, _err(ta)
        assert np.array_equal(docs_s, docs0[:total]) and np.array_equal(starts_s, starts0)
        rc, docs1, starts1 = dev.raw_docset(queries, total)
        assert rc == 0, _err(ta)
        assert np.array_equal(docs1, docs0[:total]) and np.array_equal(starts1, starts0)
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == ta.binding.KERNEL_DOCSET and st["matches"] == total, st
    finally:
        dev.close()
