"""GPU parity of the SCORED doc sets of phrase queries, phrases as boolean clauses and nested boolean queries
(tantivy_amd/csrc/tq_docset_tree_score.hip behind the option "docset_score_trees"; Weight::for_each of PhraseWeight and of
the `SpecializedScorer::Other` trees of BooleanWeight::complex_scorer): every alive matching doc, ascending, with its
score — the oracle's (O.tree_match_all / O.match_all), and bit for bit what tree_kernel gives the doc through
tq_search_batch.

Comparison rule: docs exact everywhere; tree scores within 1e-5 relative of the oracle (the project's rule for tree
scores: BASELINE.json, tests/test_gpu_tree.py); a plain TQ_MODE_PHRASE query is one IEEE bm25: bit-equal to O.match_all;
flat queries of a mixed batch by tests/test_gpu_docset_scored.py's rule.  Reference weights: one Bm25Weight per term
(default_weights(seg, [t], MODE_OR)), one per phrase on each of its terms (default_weights(seg, terms, MODE_PHRASE)), the
segment's shared cache."""
import functools
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import phrase_model as PM
from tests.helpers import alive_bytes, corpus_segment
from tests.test_gpu_docset_scored import _assert_scored, _guard_f32, _ref, _weights
from tests.test_gpu_docset_tree import _dev_query, _rows, _shape_batch, _want
from tests.test_gpu_round3 import _alive_bytes
from tests.tree_shapes import DEEP_SHAPES, PHRASE_SHAPES, SHAPES, to_device

pytestmark = pytest.mark.gpu

M, S, N = O.MUST, O.SHOULD, O.MUST_NOT
ERR_INVALID, ERR_UNSUPPORTED = 1, 4
GUARD = 0xDEADBEEF
PH = 0x10  # TQ_NESTED_PHRASE
NO_DOCS, NO_SCORES = np.zeros(0, np.uint32), np.zeros(0, np.float32)


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


def _err(ta):
    return ta.binding.lib().tq_last_error()


def _masks(ta):
    B = ta.binding
    flat = B.KERNEL_DOCSET | B.KERNEL_DOCSET_SCORE
    return flat, flat | B.KERNEL_DOCSET_TREE | B.KERNEL_DOCSET_TREE_SCORE


def _cache(seg):
    avg = float(np.float32(seg.total_num_tokens) / np.float32(seg.max_doc))
    return np.array(list(O.bm25_for_one_term(1, seg.max_doc, avg).cache), np.float32)


def _w1(seg, t):
    return float(O.default_weights(seg, [t], O.MODE_OR)[0].weight) if t < len(seg.terms) else 1.0


def _wph(seg, terms):
    if any(t >= len(seg.terms) for t in terms):
        return 1.0  # (an absent term: the phrase matches nothing, its weight is never read)
    return float(O.default_weights(seg, list(terms), O.MODE_PHRASE)[0].weight)


def _tw(ta, seg, q):
    """The weights of one query of these tests (tests/test_gpu_docset_tree.py's forms) as the device takes them."""
    if q[0] == "flat":
        return _weights(seg, [q[1]])[0][0]
    if q[0] == "phrase":
        return [_wph(seg, q[1])] * len(q[1])
    mode, terms, occurs, clause_of, msm, extra = to_device(ta, q[1], q[2])
    nested, atom_of = extra["nested_occurs"], extra["atom_of"]
    out = []
    for i, t in enumerate(terms):
        if nested[i] & PH:
            group = [terms[j] for j in range(len(terms)) if clause_of[j] == clause_of[i] and atom_of[j] == atom_of[i]]
            out.append(_wph(seg, group))
        else:
            out.append(_w1(seg, t))
    return out


def _sref(seg, q, deleted=()):
    """The oracle's ascending (docs, f32 scores) of one query, deleted docs removed."""
    if q[0] == "flat":
        return _ref(seg, q[1], deleted)
    if q[0] == "tree":
        d, s = O.tree_match_all(seg, q[1], q[2])
    else:
        d, s = O.match_all(seg, list(q[1]), O.MODE_PHRASE, phrase_offsets=list(q[2]))
    d, s = np.asarray(d, np.uint32), np.asarray(s, np.float32)
    if len(deleted):
        keep = ~np.isin(d, np.fromiter(deleted, np.uint32, len(deleted)))
        d, s = d[keep], s[keep]
    return d, s


def _check(seg, queries, docs, scores, starts, want):
    assert len(starts) == len(queries) + 1 and int(starts[0]) == 0
    for i, (q, (wd, ws)) in enumerate(zip(queries, want)):
        a, b = int(starts[i]), int(starts[i + 1])
        gd, gs = docs[a:b], scores[a:b]
        assert gd.size == wd.size and np.array_equal(gd, wd), (i, q, gd[:8], wd[:8], gd.size, wd.size)
        if q[0] == "flat":
            _assert_scored(seg, [q[1]], gd, gs, np.array([0, gd.size], np.uint64), [(wd, ws)])
        elif q[0] == "phrase":
            same = gs.view(np.uint32) == ws.view(np.uint32)
            assert np.all(same), (i, q, gd[~same][:4], gs[~same][:4], ws[~same][:4])
        else:
            rel = np.abs(gs.astype(np.float64) - ws.astype(np.float64)) / np.abs(ws.astype(np.float64))
            assert np.all(rel <= 1e-5), (i, q, gd[rel > 1e-5][:4], gs[rel > 1e-5][:4], ws[rel > 1e-5][:4], float(rel.max()))


def _run(ta, dev, seg, queries, want, guard=8, weights=None, cache=None):
    """One tq_docset_scored_batch call against `want`: rc 0, rows and scores, untouched guard words behind both arrays."""
    total = sum(w[0].size for w in want)
    weights = [_tw(ta, seg, q) for q in queries] if weights is None else weights
    rc, docs, scores, starts = dev.raw_docset_scored([_dev_query(ta, q) for q in queries], total, guard=guard, weights=weights,
                                                     cache=_cache(seg) if cache is None else cache)
    assert rc == 0, _err(ta)
    assert int(starts[-1]) == total
    _check(seg, queries, docs, scores, starts, want)
    assert np.all(docs[total:] == GUARD) and np.all(_guard_f32(scores[total:]) == GUARD)
    return docs[:total], scores[:total], starts


@functools.lru_cache(maxsize=None)
def _synth(max_doc, n_terms, segment_ord=0):
    return O.synth_segment(max_doc, n_terms=n_terms, segment_ord=segment_ord, with_positions=True)


@functools.lru_cache(maxsize=None)
def _shape_refs():
    """tests/test_gpu_docset_tree.py's mixed batch with the oracle's scores: (segment, queries, [(docs, scores)])."""
    seg, queries, want_docs, _ = _shape_batch()
    want = [_sref(seg, q) for q in queries]
    for w, wd in zip(want, want_docs):
        assert np.array_equal(w[0], wd)
    return seg, queries, want


# ---- 1. the option gate
def test_option_gate(ta):
    seg = _synth(60_000, 48)
    flat_mask, tree_mask = _masks(ta)
    good = [("flat", (O.MODE_AND, [0, 1])), ("flat", (O.MODE_OR, [2, 40]))]
    bads = [("phrase", [0, 1], [0, 1]), ("tree", [(M, 1), (M, [(M, 2), (N, 3)], 0)], 0)]
    want_good = [_sref(seg, q) for q in good]
    want_bad = [_sref(seg, q) for q in bads]
    assert all(w[0].size for w in want_bad)
    cap = sum(w[0].size for w in want_good) + max(w[0].size for w in want_bad) + 1000
    cache = _cache(seg)
    dev = ta.DeviceIndex([seg])
    try:
        def refused():
            for bad in bads:
                for at in (0, 2):  # first and last of the batch
                    batch = good[:at] + [bad] + good[at:]
                    rc, docs, scores, _ = dev.raw_docset_scored([_dev_query(ta, q) for q in batch], cap, guard=4,
                                                                weights=[_tw(ta, seg, q) for q in batch], cache=cache)
                    assert rc == ERR_UNSUPPORTED, (bad, rc, _err(ta))
                    assert ("query %d" % at).encode() in _err(ta), _err(ta)
                    assert np.all(docs == GUARD) and np.all(_guard_f32(scores) == GUARD)  # nothing was launched

        refused()  # the default
        dev.set_option("docset_trees", 1)
        refused()  # the unscored calls' option does not concern the scored ones
        dev.set_option("docset_trees", 0)
        with pytest.raises(Exception):
            dev.set_option("docset_score_trees", 2)
        refused()  # (a refused value changes nothing)
        off_docs, off_scores, off_starts = _run(ta, dev, seg, good, want_good)  # flat only, option off
        assert dev.last_batch_stats()["kernel_mask"] == flat_mask
        dev.set_option("docset_score_trees", 1)
        for bad, w in zip(bads, want_bad):
            for at in (0, 2):
                _run(ta, dev, seg, good[:at] + [bad] + good[at:], want_good[:at] + [w] + want_good[at:])
                st = dev.last_batch_stats()
                assert st["kernel_mask"] == tree_mask, st
                assert st["matches"] == sum(x[0].size for x in want_good) + w[0].size
            # ... and the unscored call still refuses it: the two options are independent
            rc, docs, _ = dev.raw_docset([_dev_query(ta, bad)], cap, guard=4)
            assert rc == ERR_UNSUPPORTED and np.all(docs == GUARD), (rc, _err(ta))
        on_docs, on_scores, on_starts = _run(ta, dev, seg, good, want_good)  # flat only, option on: as it was
        assert dev.last_batch_stats()["kernel_mask"] == flat_mask
        assert np.array_equal(on_docs, off_docs) and np.array_equal(on_starts, off_starts)
        assert np.array_equal(_guard_f32(on_scores), _guard_f32(off_scores))
        with pytest.raises(Exception):
            dev.set_option("docset_score_trees", 2)
        _run(ta, dev, seg, [bads[0]], [want_bad[0]])  # (still 1)
        dev.set_option("docset_score_trees", 0)
        refused()
    finally:
        dev.close()


# ---- 2. boundaries: hand-made lists with positions around the word, tile and segment ends
BOUNDARY_MAX_DOC = 131_113  # two tree tiles, three doc-set tiles; the last word holds 9 docs
AB_DOCS = [31, 32, 33, 63, 64, 65535, 65536, 65537, 131071, 131072, BOUNDARY_MAX_DOC - 1]
C_POS, D_POS = [0, 5, 10], [[1], [1, 6], [3], [6, 11]]


@functools.lru_cache(maxsize=None)
def _boundary_segment():
    """a b: aligned twice / once / not at all by i % 3; c d on every third doc: c has 1..3 positions, d one of four
    position sets, so "c d" aligns 0..2 times in 12 combinations; fieldnorms that vary with the doc."""
    md = BOUNDARY_MAX_DOC
    cd = list(range(0, md, 3))
    b_pos = [[1, 5], [1, 9], [2]]
    postings = [[(d, 2) for d in AB_DOCS], [(d, len(b_pos[i % 3])) for i, d in enumerate(AB_DOCS)],
                [(d, 1 + (d // 3) % 3) for d in cd], [(d, len(D_POS[(d // 3) % 4])) for d in cd]]
    positions = [[[0, 4] for _ in AB_DOCS], [b_pos[i % 3] for i in range(len(AB_DOCS))],
                 [C_POS[: 1 + (d // 3) % 3] for d in cd], [D_POS[(d // 3) % 4] for d in cd]]
    return O.build_segment(md, postings, [1 + d % 37 for d in range(md)], record_option=O.WITH_FREQS_AND_POSITIONS,
                           positions=positions)


@pytest.mark.parametrize("dense_ratio", [4096, 1 << 16])
def test_word_tile_and_segment_boundaries(ta, dense_ratio):
    """At dense_ratio 4096 the 11-doc lists a and b are reached through the probe pool's tables, at 65 536 (with
    dense_budget_x 256) every list has tables of its own."""
    seg = _boundary_segment()
    md = seg.max_doc
    _, tree_mask = _masks(ta)
    A, B, C_, D, ABSENT = 0, 1, 2, 3, 77
    ph_ab, ph_cd = ("ph", [A, B]), ("ph", [C_, D])
    queries = [("phrase", [A, B], [0, 1]), ("phrase", [C_, D], [0, 1]), ("tree", [(M, C_), (N, ph_cd)], 0),
               ("tree", [(S, ph_ab), (S, D)], 0), ("tree", [(M, ph_cd), (M, A)], 0), ("phrase", [A, ABSENT], [0, 1]),
               ("tree", [(M, A), (M, [(S, [C_, D]), (S, B)], 0)], 0)]
    # the inputs hold what they claim: phrase counts 1 and 2 for both phrases, on docs next to the boundaries
    ab2 = [d for i, d in enumerate(AB_DOCS) if i % 3 == 0]
    ab1 = [d for i, d in enumerate(AB_DOCS) if i % 3 == 1]
    assert ab2 == [31, 63, 65536, 131072] and ab1 == [32, 64, 65537, 131112]
    cd_count = lambda d: sum(1 for pd in D_POS[(d // 3) % 4] if pd - 1 in C_POS[: 1 + (d // 3) % 3])
    assert {cd_count(d) for d in range(0, md, 3)} == {0, 1, 2}
    wants = {}
    for deleted in ((), (64, 131112)):
        want = [_sref(seg, q, deleted) if i != 5 else (NO_DOCS, NO_SCORES) for i, q in enumerate(queries)]
        assert want[0][0].tolist() == sorted(set(ab2 + ab1) - set(deleted))
        assert want[1][0].size == sum(1 for d in range(0, md, 3) if cd_count(d) and d not in deleted)
        assert np.unique(want[1][1].view(np.uint32)).size > 50  # (fieldnorms and counts vary with the doc)
        assert all(w[0].size for i, w in enumerate(want) if i != 5)
        wants[deleted] = want
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", dense_ratio)
        dev.set_option("dense_budget_x", 256)
        dev.set_option("docset_score_trees", 1)
        for deleted, want in wants.items():
            dev.set_alive_bitset(_alive_bytes(md, deleted) if deleted else None)
            total = sum(w[0].size for w in want)
            _, _, starts = _run(ta, dev, seg, queries, want)
            assert starts[5] == starts[6] and starts[4] < starts[5] < starts[7]  # an empty row between non-empty ones
            st = dev.last_batch_stats()
            assert st["kernel_mask"] == tree_mask and st["matches"] == total, st
            assert dev.last_batch_match_counts(len(queries)).tolist() == [w[0].size for w in want]
        n_own = sum(1 for t in seg.terms[:4] if t.doc_freq * dense_ratio >= md)
        assert n_own == (4 if dense_ratio == 1 << 16 else 2)
        assert dev.segment_stats(0)["n_dense_lists"] == n_own
    finally:
        dev.close()


# ---- 3. every shape of tests/tree_shapes.py, plain phrases and flat queries in one batch
def test_every_shape_equals_the_oracle(ta):
    seg, queries, want = _shape_refs()
    flat_mask, tree_mask = _masks(ta)
    trees = [i for i, q in enumerate(queries) if q[0] != "flat"]
    assert sum(1 for q in queries if q[0] == "tree") == 69 and len(trees) == 72  # (+ the three plain phrases)
    assert all(want[i][0].size for i in trees)  # every such row scores something
    assert min(float(want[i][1].min()) for i in trees) > 0.4
    flat_only = [q for q in queries if q[0] == "flat"]
    flat_want = [w for q, w in zip(queries, want) if q[0] == "flat"]
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("docset_score_trees", 1)
        docs, scores, starts = _run(ta, dev, seg, queries, want)
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == tree_mask, st
        assert st["matches"] == sum(w[0].size for w in want)
        assert dev.last_batch_match_counts(len(queries)).tolist() == [w[0].size for w in want]
        # the flat queries of the mixed batch: bit for bit what a flat-only call gives them
        fdocs, fscores, fstarts = _run(ta, dev, seg, flat_only, flat_want, guard=0)
        assert dev.last_batch_stats()["kernel_mask"] == flat_mask
        at = 0
        for i, q in enumerate(queries):
            if q[0] != "flat":
                continue
            a, b, fa, fb = int(starts[i]), int(starts[i + 1]), int(fstarts[at]), int(fstarts[at + 1])
            assert np.array_equal(docs[a:b], fdocs[fa:fb]) and np.array_equal(_guard_f32(scores[a:b]), _guard_f32(fscores[fa:fb])), i
            at += 1
    finally:
        dev.close()


# ---- 4. one score per doc, whichever entry point
def test_scores_are_tree_kernels_bit_for_bit(ta):
    seg, queries, want = _shape_refs()
    B = ta.binding
    K = 1024
    trees = [i for i, q in enumerate(queries) if q[0] != "flat"]
    in_range = [i for i in trees if 1 <= want[i][0].size <= K]
    assert len(in_range) >= 20, len(in_range)
    cache = _cache(seg)
    avg2 = 3.0 * float(np.float32(seg.total_num_tokens) / np.float32(seg.max_doc))  # another average fieldnorm
    cache2 = np.array(list(O.bm25_for_one_term(1, seg.max_doc, avg2).cache), np.float32)
    assert not np.array_equal(cache, cache2)
    weights = [_tw(ta, seg, q) for q in queries]
    dq = [_dev_query(ta, q) for q in queries]
    total = sum(w[0].size for w in want)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("docset_score_trees", 1)
        dev.set_option("record_query_kernels", 1)
        for second in (False, True):
            # second run: every other query — flat and tree alike — under a second tf_cache, the mixed batch in one call
            caches = [cache2 if second and i % 2 else cache for i in range(len(queries))]
            if second:
                rc, docs, scores, starts = dev.raw_docset_scored(dq, total, weights=weights, cache=caches)
                assert rc == 0, _err(ta)
                assert all(np.array_equal(docs[int(starts[i]): int(starts[i + 1])], want[i][0]) for i in range(len(queries)))
            else:
                docs, scores, starts = _run(ta, dev, seg, queries, want)
            sc, dc, ct = dev.raw_search_trees([dq[i] for i in trees], [weights[i] for i in trees], [caches[i] for i in trees],
                                              K, (1, B.OPT_DEFAULT))
            kern = dev.last_batch_query_kernels(len(trees))
            n_checked = 0
            for at, i in enumerate(trees):
                n = want[i][0].size
                if not (1 <= n <= K) or int(kern[at]) != B.KERNEL_TREE:
                    continue
                assert int(ct[at]) == n, (i, int(ct[at]), n)
                order = np.argsort(dc[at, :n], kind="stable")
                a = int(starts[i])
                assert np.array_equal(dc[at, :n][order], docs[a: a + n]), i
                same = sc[at, :n][order].view(np.uint32) == scores[a: a + n].view(np.uint32)
                assert np.all(same), (i, queries[i], docs[a: a + n][~same][:4], sc[at, :n][order][~same][:4], scores[a: a + n][~same][:4])
                n_checked += 1
            assert n_checked >= 10, n_checked
            if second:  # the scores under the second cache differ from the first run's: the cache index is the query's own
                i = next(i for i in in_range if i % 2)
                a, b = int(starts[i]), int(starts[i + 1])
                assert not np.array_equal(_guard_f32(scores[a:b]), _guard_f32(want[i][1]))
                i = next(i for i in in_range if i % 2 == 0)
                a, b = int(starts[i]), int(starts[i + 1])
                assert np.allclose(scores[a:b], want[i][1], rtol=1e-5, atol=0)
    finally:
        dev.close()


# ---- 5. capacity protocol, sub-batches, device variant
def test_capacity_sub_batches_and_device_variant(ta):
    import torch

    seg, queries, want = _shape_refs()
    _, tree_mask = _masks(ta)
    dq = [_dev_query(ta, q) for q in queries]
    weights = [_tw(ta, seg, q) for q in queries]
    cache = _cache(seg)
    total, n = sum(w[0].size for w in want), len(queries)
    assert sum(1 for q in queries if q[0] != "flat") > 3 * 16  # more result slots than three sub-batches of 16 hold
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("docset_score_trees", 1)
        docs_d, scores_d, starts_d = _run(ta, dev, seg, queries, want)
        dev.set_option("docset_temp_lists", 16)
        docs_s, scores_s, starts_s = _run(ta, dev, seg, queries, want)
        assert np.array_equal(starts_s, starts_d) and np.array_equal(docs_s, docs_d)
        assert np.array_equal(_guard_f32(scores_s), _guard_f32(scores_d))
        assert dev.last_batch_match_counts(n).tolist() == [w[0].size for w in want]
        for lists in (16, 0):  # host variant, one entry short: the row starts complete, no doc and no score written
            dev.set_option("docset_temp_lists", lists)
            rc, docs2, scores2, starts2 = dev.raw_docset_scored(dq, total - 1, guard=65, weights=weights, cache=cache)
            assert rc == ERR_INVALID and _err(ta)
            assert np.array_equal(starts2, starts_d)
            assert np.all(docs2 == GUARD) and np.all(_guard_f32(scores2) == GUARD)
        # device variant, half the room: nothing at or past out_cap in either tensor, the full total in d_out_starts[n]
        guard32 = np.array([GUARD], np.uint32).view(np.int32)[0]
        for lists in (0, 16):
            dev.set_option("docset_temp_lists", lists)
            cap = total // 2
            d_docs = torch.full((total + 64,), int(guard32), dtype=torch.int32, device="cuda")
            d_scores = torch.full((total + 64,), int(guard32), dtype=torch.int32, device="cuda").view(torch.float32)
            d_starts = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            rc = dev.raw_docset_scored_device(dq, d_docs, d_scores, cap, d_starts, weights=weights, cache=cache)
            assert rc == 0, _err(ta)
            st = dev.last_batch_stats()  # (waits for the batch)
            torch.cuda.synchronize()
            docs = d_docs.cpu().numpy().view(np.uint32)
            scores = d_scores.cpu().numpy()
            starts = d_starts.cpu().numpy()
            assert int(starts[n]) == total and np.array_equal(starts.astype(np.uint64), starts_d)
            assert np.array_equal(docs[:cap], docs_d[:cap])
            assert np.array_equal(_guard_f32(scores[:cap]), _guard_f32(scores_d[:cap]))
            assert np.all(docs[cap:] == GUARD) and np.all(_guard_f32(scores[cap:]) == GUARD)
            assert st["kernel_mask"] == tree_mask and st["matches"] == total, st
    finally:
        dev.close()


# ---- 6. refusals with the option on
def test_refusals_leave_the_segment_usable(ta):
    docs = ["a b c d e f g h x", "a b c d e f g h", "h g f e d c b a x", "x a b c d e f g h y a b c d e f g h", "a b c d x e f g h"] * 40
    docs += ["x y", "a x", "b c d"] * 30
    seg, v = corpus_segment(docs)
    ph8 = ("ph", [v[w] for w in "abcdefgh"])
    good = [("tree", [(M, ph8), (M, v["x"])], 0), ("flat", (O.MODE_OR, [v["x"], v["y"]])),
            ("tree", [(M, v["a"]), (M, [(S, ph8), (S, v["y"])], 0)], 0)]
    want = [_sref(seg, q) for q in good]
    assert all(w[0].size >= 30 for w in want)
    nested = ("tree", [(M, v["a"]), (M, [(M, v["b"]), (N, v["x"])], 0)], 0)
    nine = ("phrase", [v[w] for w in "abcdefghx"], list(range(9)))
    cache = _cache(seg)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("docset_score_trees", 1)
        _run(ta, dev, seg, good, want)
        cases = [(nested, "weights", ERR_INVALID), (nested, "cache", ERR_INVALID), (nested, "nan", ERR_INVALID),
                 (nine, None, ERR_UNSUPPORTED), (nested, "negative", ERR_UNSUPPORTED)]
        for bad, what, code in cases:
            for at in (0, 3):
                batch = good[:at] + [bad] + good[at:]
                weights = [_tw(ta, seg, q) for q in batch]
                caches = [cache] * len(batch)
                if what == "weights":
                    weights[at] = None
                elif what == "cache":
                    caches[at] = None
                elif what == "nan":
                    weights[at] = [weights[at][0], float("nan")] + weights[at][2:]
                elif what == "negative":
                    weights[at] = [weights[at][0], -weights[at][1]] + weights[at][2:]
                rc, out, sc, _ = dev.raw_docset_scored([_dev_query(ta, q) for q in batch], 100_000, guard=4, weights=weights,
                                                       cache=caches)
                assert rc == code, (what, rc, _err(ta))
                assert ("query %d" % at).encode() in _err(ta), _err(ta)
                assert np.all(out == GUARD) and np.all(_guard_f32(sc) == GUARD)  # nothing was launched
                _run(ta, dev, seg, good, want)  # the segment stays usable
    finally:
        dev.close()


# ---- 7. phrase counts at the codec's edges: tests/phrase_model.py's corpora, through the host mirror
EXTRA = 7  # the term of `+"..." +c`


def _as_clause(terms, offs, extra=None):
    """The phrase as the only Must clause of a boolean query, or `+"..." +extra`."""
    n = len(terms)
    if extra is None:
        return (O.MODE_BOOL, list(terms), [M] * n, [0] * n, 0,
                {"nested_occurs": [M | PH] * n, "atom_of": [0] * n, "phrase_offsets": list(offs)})
    return (O.MODE_BOOL, list(terms) + [extra], [M] * (n + 1), [0] * n + [1], 0,
            {"nested_occurs": [M | PH] * n + [M], "atom_of": [0] * (n + 1), "phrase_offsets": list(offs) + [0]})


def _term_scores(corp, t, docs):
    """float64 BM25 of the single term t on `docs`."""
    n = len(corp.tp[t])
    w = (1.0 + PM.K1) * math.log(1.0 + (corp.max_doc - n + 0.5) / (n + 0.5))
    avgdl = sum(corp.fieldnorms) / corp.max_doc
    return np.array([PM.bm25(w, len(corp.tp[t][int(d)]), float(corp.fieldnorms[int(d)]), avgdl) for d in docs], np.float64)


@pytest.mark.parametrize("name", PM.CORPORA)
def test_phrase_counts_at_the_codecs_edges(ta, name):
    corp = PM.corpus(name)
    B = ta.binding
    nq = len(corp.queries)
    queries = [(O.MODE_PHRASE, terms, offs) for _, terms, offs in corp.queries]
    queries += [_as_clause(terms, offs) for _, terms, offs in corp.queries]
    queries += [_as_clause(terms, offs, EXTRA) for _, terms, offs in corp.queries]
    assert int(np.sum(corp.expect(PM.MAIN)[2] >= 2)) >= 6  # docs where the phrase lines up more than once
    dev = ta.DeviceIndex([corp.segment()])
    try:
        dev.set_option("dense_budget_x", 256)
        dev.set_option("docset_score_trees", 1)
        if corp.deleted is not None:
            dev.set_alive_bitset(alive_bytes(corp.max_doc, corp.deleted))
        got = dev.docset_scored(queries)
        st = dev.last_batch_stats()
        assert st["kernel_mask"] & B.KERNEL_DOCSET_TREE_SCORE, st

        def same(at, qname, wd, ws):
            pairs, gs = got[at]
            assert np.all(pairs[:, 0] == 0)
            assert np.array_equal(pairs[:, 1], wd), (corp.name, qname, pairs[:8, 1], wd[:8], pairs.shape[0], wd.size)
            rel = np.abs(gs.astype(np.float64) - ws) / np.maximum(np.abs(ws), 1e-30)
            assert np.all(rel <= 1e-5), (corp.name, qname, wd[rel > 1e-5][:8], gs[rel > 1e-5][:8], ws[rel > 1e-5][:8])

        n_both = 0
        for qi, (qname, terms, offs) in enumerate(corp.queries):
            wd, ws, _ = corp.expect(qi)
            same(qi, qname, wd, ws)
            same(nq + qi, "+" + qname, wd, ws)
            has = np.array([int(d) in corp.tp[EXTRA] for d in wd], bool)
            same(2 * nq + qi, qname + " +c", wd[has], ws[has] + _term_scores(corp, EXTRA, wd[has]))
            n_both += int(has.sum())
        assert n_both >= 20
    finally:
        dev.close()


# ---- 8. host mirror
MIRROR_QUERIES = [("tree", PHRASE_SHAPES[0][0](list(range(8))), 0), ("tree", PHRASE_SHAPES[6][0](list(range(8))), 2),
                  ("tree", PHRASE_SHAPES[8][0](list(range(8))), 0), ("tree", SHAPES[0][0](list(range(8, 16))), 0),
                  ("tree", SHAPES[7][0](list(range(8, 16))), 0), ("tree", DEEP_SHAPES[4][0](list(range(8, 16))), 0),
                  ("tree", PHRASE_SHAPES[5][0](list(range(8, 16))), 0), ("tree", PHRASE_SHAPES[7][0](list(range(8, 16))), 0)]


def test_host_mirror_one_segment(ta):
    seg = _synth(70_000, 48)
    queries = MIRROR_QUERIES + [("phrase", [0, 1], [0, 1]), ("tree", SHAPES[3][0](list(range(8))), 0)]
    dq = [_dev_query(ta, q) for q in queries]
    dev = ta.DeviceIndex([seg])
    try:
        with pytest.raises(Exception):  # the default: refused
            dev.docset_scored(dq)
        dev.set_option("docset_score_trees", 1)
        dev.set_option("docset_trees", 1)
        got = dev.docset_scored(dq)
        plain = dev.docset(dq)
        for q, (g, gs), pl in zip(queries, got, plain):
            wd, ws = _sref(seg, q)
            assert wd.size and g.dtype == np.uint32 and np.array_equal(g, pl), q
            assert np.all(g[:, 0] == 0) and np.array_equal(g[:, 1], wd), q
            assert gs.dtype == np.float32 and np.allclose(gs, ws, rtol=1e-5, atol=0), q
        assert np.array_equal(dev.count(dq), np.array([g.shape[0] for g, _ in got], np.uint64))
    finally:
        dev.close()


def test_host_mirror_two_segments_equal_the_exhaustive_search(ta):
    K = 1024
    segs = [_synth(70_000, 48, 0), _synth(83_001, 48, 1)]
    queries = MIRROR_QUERIES
    for q in queries:
        assert all(1 <= _want(s, q).size <= K for s in segs), q
    dq = [_dev_query(ta, q) for q in queries]
    dev = ta.DeviceIndex(segs)
    try:
        dev.set_option("docset_score_trees", 1)  # (on both segments)
        got = dev.docset_scored(dq)
        for q, (g, gs) in zip(queries, got):
            w0, w1 = _want(segs[0], q), _want(segs[1], q)
            want = np.concatenate([np.stack([np.zeros_like(w0), w0], axis=1), np.stack([np.ones_like(w1), w1], axis=1)])
            assert g.shape == want.shape and np.array_equal(g, want), q
        assert np.array_equal(dev.count(dq), np.array([g.shape[0] for g, _ in got], np.uint64))
        dev.set_option("exhaustive", 1)
        scores, ords, docs, counts = dev.search(dq, K)
        for i, (q, (g, gs)) in enumerate(zip(queries, got)):
            order = np.lexsort((g[:, 1], g[:, 0], -gs.astype(np.float64)))[:K]
            c = int(counts[i])
            assert c == order.size, (q, c, order.size)
            assert np.array_equal(ords[i, :c], g[order, 0]) and np.array_equal(docs[i, :c], g[order, 1]), q
            assert np.array_equal(scores[i, :c].view(np.uint32), gs[order].view(np.uint32)), q
    finally:
        dev.close()


# ---- 9. small segments
WORDS = "a b c d e f g h i j k l".split()


@pytest.mark.parametrize("seeds", [list(range(g * 10, g * 10 + 10)) for g in range(4)])
def test_fuzz_small_segments(ta, seeds):
    """tests/test_gpu_docset_tree.py::test_fuzz_small_segments' generator: segments below 4096 docs get no tables of
    their own and take the probe pool's."""
    shapes = SHAPES + DEEP_SHAPES + PHRASE_SHAPES
    _, tree_mask = _masks(ta)
    for seed in seeds:
        rng = np.random.default_rng(9000 + seed)
        n_docs = int(rng.integers(200, 5001))
        p = 1.0 / np.arange(1, len(WORDS) + 1)
        p /= p.sum()
        lens = rng.integers(1, 9, size=n_docs)
        toks = rng.choice(len(WORDS), size=int(lens.sum()), p=p)
        ends = np.cumsum(lens)
        docs = [" ".join(WORDS)] + [" ".join(WORDS[t] for t in toks[e - l: e]) for e, l in zip(ends[1:], lens[1:])]
        seg, v = corpus_segment(docs)
        assert len(v) == len(WORDS)
        queries = []
        for _ in range(12):
            shape, msm = shapes[int(rng.integers(len(shapes)))]
            queries.append(("tree", shape(rng.permutation(len(WORDS))[:8].tolist()), msm))
        want = [_sref(seg, q) for q in queries]
        dev = ta.DeviceIndex([seg])
        try:
            dev.set_option("docset_score_trees", 1)
            _run(ta, dev, seg, queries, want)
            assert dev.last_batch_stats()["kernel_mask"] == tree_mask
        finally:
            dev.close()
