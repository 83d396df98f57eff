"""GPU parity of the doc sets of phrase queries, phrases as boolean clauses and nested boolean queries
(tantivy_amd/csrc/tq_docset_tree.hip behind the option "docset_trees"; Weight::for_each_no_score of PhraseWeight and of
the `SpecializedScorer::Other` trees of BooleanWeight::complex_scorer): every alive matching doc, ascending, as CSR
rows — exactly the oracle's doc sets (O.tree_match_all / O.match_all / O.bool_match_all).  Covers the option gate, the
word / tile / segment-tail boundaries, every shape of tests/tree_shapes.py mixed with flat queries, the capacity
protocol and sub-batching, the tree path's limits, small random segments, the host mirror and the scored refusal."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import corpus_segment
from tests.test_gpu_round3 import _alive_bytes
from tests.tree_shapes import DEEP_SHAPES, PHRASE_SHAPES, SHAPES, to_device, wide_minimum

pytestmark = pytest.mark.gpu

M, S, N = O.MUST, O.SHOULD, O.MUST_NOT
ERR_INVALID, ERR_UNSUPPORTED = 1, 4
GUARD = 0xDEADBEEF
EMPTY = np.zeros(0, np.uint32)


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


def _err(ta):
    return ta.binding.lib().tq_last_error()


# A query of these tests: ("tree", spec, msm) — tests/tree_shapes.py's clause-list form; ("phrase", term ids, offsets) —
# a plain TQ_MODE_PHRASE query; ("flat", device tuple) — what tests/test_gpu_docset.py sends.
def _dev_query(ta, q):
    if q[0] == "tree":
        return to_device(ta, q[1], q[2])
    if q[0] == "phrase":
        return (O.MODE_PHRASE, list(q[1]), list(q[2]))
    return q[1]


def _want(seg, q, deleted=()):
    """The oracle's ascending doc set of one query, deleted docs removed."""
    if q[0] == "tree":
        d = O.tree_match_all(seg, q[1], q[2])[0]
    elif q[0] == "phrase":
        d = O.match_all(seg, list(q[1]), O.MODE_PHRASE, phrase_offsets=list(q[2]))[0]
    else:
        f = q[1]
        if f[0] == O.MODE_BOOL:
            d = O.bool_match_all(seg, f[1], f[2], f[3] if len(f) > 3 else None, f[4] if len(f) > 4 else 0)[0]
        else:
            d = O.match_all(seg, f[1], f[0])[0]
    d = np.asarray(d, np.uint32)
    if len(deleted):
        d = d[~np.isin(d, np.fromiter(deleted, np.uint32, len(deleted)))]
    return d


def _rows(docs, starts):
    return [docs[int(starts[q]): int(starts[q + 1])] for q in range(len(starts) - 1)]


def _assert_rows(queries, got, want, max_doc):
    assert len(got) == len(want)
    for q, g, w in zip(queries, got, want):
        assert g.size == w.size and np.array_equal(g, w), (q, g[:8], w[:8], g.size, w.size)
        assert np.all(np.diff(g.astype(np.int64)) > 0), q
        assert g.size == 0 or int(g[-1]) < max_doc, q


def _run(ta, dev, queries, want, max_doc, guard=8):
    """One tq_docset_batch call over `queries` against `want`: rc 0, exact ascending rows, untouched guard words."""
    total = sum(w.size for w in want)
    rc, docs, starts = dev.raw_docset([_dev_query(ta, q) for q in queries], total, guard=guard)
    assert rc == 0, _err(ta)
    assert int(starts[0]) == 0 and int(starts[-1]) == total
    _assert_rows(queries, _rows(docs, starts), want, max_doc)
    assert np.all(docs[total:] == GUARD)
    return docs, starts


@functools.lru_cache(maxsize=None)
def _synth(max_doc, n_terms, segment_ord=0):
    return O.synth_segment(max_doc, n_terms=n_terms, segment_ord=segment_ord, with_positions=True)


# ---- 1. the option gate
def test_option_gate(ta):
    seg = _synth(60_000, 48)
    good = [(O.MODE_AND, [0, 1]), (O.MODE_OR, [2, 40])]
    phrase = (O.MODE_PHRASE, [0, 1], [0, 1])
    nested = (ta.MODE_BOOL, [1, 2, 3], [M, M, M], [0, 1, 1], 0, {"nested_occurs": [M, M, N]})
    want_good = [_want(seg, ("flat", q)) for q in good]
    want_phrase = _want(seg, ("phrase", [0, 1], [0, 1]))
    want_nested = _want(seg, ("tree", [(M, 1), (M, [(M, 2), (N, 3)], 0)], 0))
    assert want_phrase.size and want_nested.size
    cap = sum(w.size for w in want_good) + want_phrase.size + want_nested.size + 1000
    dev = ta.DeviceIndex([seg])
    try:
        def refused():
            for bad in (phrase, nested):
                for at in (0, 2):  # first and last of the batch
                    rc, docs, _ = dev.raw_docset(good[:at] + [bad] + good[at:], cap, guard=4)
                    assert rc == ERR_UNSUPPORTED, (bad, rc, _err(ta))
                    assert ("query %d" % at).encode() in _err(ta), _err(ta)
                    assert np.all(docs == GUARD)  # nothing was launched

        refused()  # the default: as tests/test_gpu_docset.py pins it
        with pytest.raises(Exception):
            dev.set_option("docset_trees", 2)
        refused()  # (a refused value changes nothing)
        dev.set_option("docset_trees", 1)
        for bad, w in ((phrase, want_phrase), (nested, want_nested)):
            for at in (0, 2):
                rc, docs, starts = dev.raw_docset(good[:at] + [bad] + good[at:], cap, guard=4)
                assert rc == 0, _err(ta)
                want = want_good[:at] + [w] + want_good[at:]
                _assert_rows(list(range(3)), _rows(docs, starts), want, seg.max_doc)
                assert dev.last_batch_stats()["kernel_mask"] == ta.binding.KERNEL_DOCSET | ta.binding.KERNEL_DOCSET_TREE
        dev.set_option("docset_trees", 0)
        refused()
        rc, docs, starts = dev.raw_docset(good, cap)
        assert rc == 0, _err(ta)
        _assert_rows(good, _rows(docs, starts), want_good, seg.max_doc)
    finally:
        dev.close()


# ---- 2. boundaries: hand-made lists with positions around the word, tile and segment ends
BOUNDARY_MAX_DOC = 131_113  # two tree tiles, three doc-set tiles; the last word holds 9 docs
AB_DOCS = [31, 32, 33, 63, 64, 65535, 65536, 65537, 131071, 131072, BOUNDARY_MAX_DOC - 1]


@functools.lru_cache(maxsize=None)
def _boundary_segment():
    md = BOUNDARY_MAX_DOC
    cd = list(range(0, md, 3))
    postings = [[(d, 1) for d in AB_DOCS], [(d, 1) for d in AB_DOCS], [(d, 2) for d in cd], [(d, 1) for d in cd]]
    positions = [[[0] for _ in AB_DOCS], [[1] if i % 2 == 0 else [2] for i in range(len(AB_DOCS))],
                 [[0, 5] for _ in cd], [[1] if (d // 3) % 2 == 0 else [3] for d in cd]]
    return O.build_segment(md, postings, [7] * md, record_option=O.WITH_FREQS_AND_POSITIONS, positions=positions)


@pytest.mark.parametrize("dense_ratio", [4096, 1 << 16])
def test_word_tile_and_segment_boundaries(ta, dense_ratio):
    """At dense_ratio 4096 the 11-doc lists a and b are reached through the probe pool's tables, at 65 536 (with
    dense_budget_x 256) every list has tables of its own."""
    seg = _boundary_segment()
    md = seg.max_doc
    A, B, C_, D, ABSENT = 0, 1, 2, 3, 77
    ph_ab, ph_cd = ("ph", [A, B]), ("ph", [C_, D])
    queries = [("phrase", [A, B], [0, 1]), ("phrase", [C_, D], [0, 1]), ("tree", [(M, C_), (N, ph_cd)], 0),
               ("tree", [(S, ph_ab), (S, D)], 0), ("phrase", [A, ABSENT], [0, 1]), ("tree", [(M, ph_cd), (M, A)], 0)]
    cd = np.arange(0, md, 3, dtype=np.uint32)
    cd_hit = cd[(cd // 3) % 2 == 0]
    ab_hit = np.asarray(AB_DOCS[0::2], np.uint32)
    assert ab_hit.tolist() == [31, 33, 64, 65536, 131071, 131112]
    assert cd_hit.size == 21_853 and cd_hit[-3:].tolist() == [131100, 131106, 131112]
    want = [ab_hit, cd_hit, cd[(cd // 3) % 2 == 1], np.union1d(ab_hit, cd), EMPTY, np.intersect1d(cd_hit, np.asarray(AB_DOCS, np.uint32))]
    for i in (0, 1, 2, 3, 5):  # the expectations above against the oracle (it does not take an absent term)
        assert np.array_equal(_want(seg, queries[i]), want[i]), i
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", dense_ratio)
        dev.set_option("dense_budget_x", 256)
        dev.set_option("docset_trees", 1)
        for deleted in ((), (64, 131112)):
            dev.set_alive_bitset(_alive_bytes(md, deleted) if deleted else None)
            w = [x[~np.isin(x, np.asarray(deleted, np.uint32))] for x in want]
            total = sum(x.size for x in w)
            docs, starts = _run(ta, dev, queries, w, md)
            assert _rows(docs, starts)[4].size == 0  # an empty row between non-empty ones
            st = dev.last_batch_stats()
            assert st["kernel_mask"] == ta.binding.KERNEL_DOCSET | ta.binding.KERNEL_DOCSET_TREE, st
            assert st["matches"] == total, st
            assert dev.last_batch_match_counts(len(queries)).tolist() == [x.size for x in w]
        n_own = sum(1 for t in seg.terms[:4] if t.doc_freq * dense_ratio >= md)
        assert n_own == (4 if dense_ratio == 1 << 16 else 2)
        assert dev.segment_stats(0)["n_dense_lists"] == n_own
    finally:
        dev.close()


# ---- 3. every shape of tests/tree_shapes.py, plain phrases and flat queries in one batch
SHAPE_MAX_DOC = 140_000


@functools.lru_cache(maxsize=None)
def _shape_batch():
    """-> (segment, queries, oracle rows, indices of the phrase-shape queries per shape)"""
    seg = _synth(SHAPE_MAX_DOC, 48)
    rng = np.random.default_rng(77)
    queries, phrase_at = [], [[] for _ in PHRASE_SHAPES]
    flat = [("flat", (O.MODE_AND, [0, 1])), ("flat", (O.MODE_OR, [3, 41, 17])), ("flat", (O.MODE_BOOL, [2, 5, 9], [M, S, N])),
            ("flat", (O.MODE_BOOL, [4, 6, 7, 8], [S, S, S, S], None, 2)), ("flat", (O.MODE_AND, [30, 45])),
            ("flat", (O.MODE_BOOL, [1, 12, 13], [M, M, M], [0, 1, 1]))]
    for draw in range(3):
        ids = rng.permutation(40)[:8].tolist()
        for shape, msm in SHAPES + DEEP_SHAPES:
            queries.append(("tree", shape(ids), msm))
        queries.append(flat[2 * draw])
        pids = list(range(8)) if draw == 0 else rng.permutation(8).tolist()
        for si, (shape, msm) in enumerate(PHRASE_SHAPES):
            phrase_at[si].append(len(queries))
            queries.append(("tree", shape(pids), msm))
        queries.append(flat[2 * draw + 1])
    for n in (2, 3, 4):
        queries.append(("phrase", list(range(n)), list(range(n))))
    want = [_want(seg, q) for q in queries]
    return seg, queries, want, phrase_at


def test_every_shape_equals_the_oracle(ta):
    seg, queries, want, phrase_at = _shape_batch()
    # the batch exercises what it claims to: every phrase shape matches somewhere, and positions decide
    for si, at in enumerate(phrase_at):
        assert max(want[i].size for i in at) > 0, si
    and_set = _want(seg, ("flat", (O.MODE_AND, [0, 1])))
    phrase_set = _want(seg, ("phrase", [0, 1], [0, 1]))
    assert 0 < phrase_set.size < and_set.size, (phrase_set.size, and_set.size)
    flat_only = [q for q in queries if q[0] == "flat"]
    flat_want = [w for q, w in zip(queries, want) if q[0] == "flat"]
    dev = ta.DeviceIndex([seg])
    try:
        rc, off_docs, off_starts = dev.raw_docset([q[1] for q in flat_only], sum(w.size for w in flat_want))
        assert rc == 0, _err(ta)
        dev.set_option("docset_trees", 1)
        _run(ta, dev, queries, want, seg.max_doc)
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == ta.binding.KERNEL_DOCSET | ta.binding.KERNEL_DOCSET_TREE, st
        assert st["matches"] == sum(w.size for w in want)
        assert dev.last_batch_match_counts(len(queries)).tolist() == [w.size for w in want]
        # a flat-only batch with the option on: no bits kernel, the rows of the option-off run
        on_docs, on_starts = _run(ta, dev, flat_only, flat_want, seg.max_doc, guard=0)
        assert dev.last_batch_stats()["kernel_mask"] == ta.binding.KERNEL_DOCSET
        assert np.array_equal(on_docs, off_docs) and np.array_equal(on_starts, off_starts)
    finally:
        dev.close()


# ---- 4. capacity protocol and sub-batches
def test_capacity_and_sub_batches(ta):
    import torch

    seg, queries, want, _ = _shape_batch()
    dq = [_dev_query(ta, q) for q in queries]
    total, n = sum(w.size for w in want), len(queries)
    n_trees = sum(1 for q in queries if q[0] != "flat")
    assert n_trees > 3 * 16  # more result slots than a sub-batch of 16 holds
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("docset_trees", 1)
        docs_d, starts_d = _run(ta, dev, queries, want, seg.max_doc)
        dev.set_option("docset_temp_lists", 16)
        docs_s, starts_s = _run(ta, dev, queries, want, seg.max_doc)
        assert np.array_equal(starts_s, starts_d) and np.array_equal(docs_s, docs_d)
        assert dev.last_batch_match_counts(n).tolist() == [w.size for w in want]
        for lists in (16, 0):  # host variant, one doc short: the row starts complete, no doc written
            dev.set_option("docset_temp_lists", lists)
            rc, docs2, starts2 = dev.raw_docset(dq, total - 1, guard=65)
            assert rc == ERR_INVALID and _err(ta)
            assert np.array_equal(starts2, starts_d)
            assert np.all(docs2 == GUARD)
        # device variant, half the room: nothing at or past out_cap, the full total in d_out_starts[n]
        flat = np.concatenate(want)
        guard32 = np.array([GUARD], np.uint32).view(np.int32)[0]
        for lists in (0, 16):
            dev.set_option("docset_temp_lists", lists)
            cap = total // 2
            d_docs = torch.full((total + 64,), int(guard32), dtype=torch.int32, device="cuda")
            d_starts = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            rc = dev.raw_docset_device(dq, d_docs, cap, d_starts)
            assert rc == 0, _err(ta)
            st = dev.last_batch_stats()  # (waits for the batch)
            torch.cuda.synchronize()
            docs = d_docs.cpu().numpy().view(np.uint32)
            starts = d_starts.cpu().numpy()
            assert int(starts[n]) == total and np.array_equal(starts.astype(np.uint64), starts_d)
            assert np.array_equal(docs[:cap], flat[:cap])
            assert np.all(docs[cap:] == GUARD)
            assert st["kernel_mask"] == ta.binding.KERNEL_DOCSET | ta.binding.KERNEL_DOCSET_TREE and st["matches"] == total, st
    finally:
        dev.close()


# ---- 5. the limits of the tree path
def test_limits(ta):
    docs = ["a b c d e f g h x", "a b c d e f g h", "h g f e d c b a x", "x a b c d e f g h y a b c d e f g h", "a b c d x e f g h"] * 40
    docs += ["x y", "a x", "b c d"] * 30
    seg, v = corpus_segment(docs)
    ph = ("ph", [v[w] for w in "abcdefgh"])
    queries = [("tree", [(M, ph), (M, v["x"])], 0), ("tree", [(S, ph), (S, v["y"])], 0), ("tree", [(M, v["x"]), (N, ph)], 0),
               ("tree", [(M, v["a"]), (M, [(S, ph), (S, v["y"])], 0)], 0), ("phrase", ph[1], list(range(8)))]
    want = [_want(seg, q) for q in queries]
    assert all(w.size >= 30 for w in want), [w.size for w in want]
    nine = (O.MODE_PHRASE, [v[w] for w in "abcdefghx"], list(range(9)))
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("docset_trees", 1)
        _run(ta, dev, queries, want, seg.max_doc)
        dq = [_dev_query(ta, q) for q in queries]
        rc, out, _ = dev.raw_docset(dq[:1] + [nine] + dq[1:], 100_000, guard=4)
        assert rc == ERR_UNSUPPORTED and b"query 1" in _err(ta), (rc, _err(ta))
        assert np.all(out == GUARD)  # nothing was launched
        _run(ta, dev, queries, want, seg.max_doc)  # the segment stays usable
    finally:
        dev.close()
    # 16 Should terms, at least 15 / 1 of them: a doc that holds all 16 stays in (the bit-sliced counter saturates at 15)
    md = 20_011
    lists = []
    for i in range(16):
        held = sorted(set(range(0, md, 97)) | set(range(i, md, 5 + i)))
        lists.append([(d, 1 + (d + i) % 3) for d in held])
    seg16 = O.build_segment(md, lists, [5 + d % 40 for d in range(md)])
    t16 = list(range(16))
    queries = [("tree", wide_minimum(t16, 15), 0), ("tree", wide_minimum(t16, 1), 0)]
    want = [_want(seg16, q) for q in queries]
    assert np.all(np.isin(np.arange(0, md, 97, dtype=np.uint32), want[0])) and want[0].size < want[1].size
    dev = ta.DeviceIndex([seg16])
    try:
        dev.set_option("docset_trees", 1)
        _run(ta, dev, queries, want, md)
    finally:
        dev.close()


# ---- 6. small segments and fuzz
_EXTRA = int(os.environ.get("TQ_FUZZ_EXTRA", "0"))  # n more segments (a soak run, as for the other fuzz tests)
WORDS = "a b c d e f g h i j k l".split()


@pytest.mark.parametrize("seeds", [list(range(g * 10, g * 10 + 10)) for g in range(4)] + [[1000 + i] for i in range(_EXTRA)])
def test_fuzz_small_segments(ta, seeds):
    """Segments below 4096 docs get no tables of their own and take the probe pool's only for nested queries."""
    shapes = SHAPES + DEEP_SHAPES + PHRASE_SHAPES
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
        want = [_want(seg, q) for q in queries]
        dev = ta.DeviceIndex([seg])
        try:
            dev.set_option("docset_trees", 1)
            _run(ta, dev, queries, want, seg.max_doc)
        finally:
            dev.close()


# ---- 7. host mirror over two segments
def test_host_mirror_over_two_segments(ta):
    segs = [_synth(70_000, 48, 0), _synth(83_001, 48, 1)]
    ids = [0, 1, 2, 3, 4, 5, 6, 7]
    queries = [("phrase", [0, 1], [0, 1]), ("tree", PHRASE_SHAPES[0][0](ids), PHRASE_SHAPES[0][1]),
               ("tree", SHAPES[0][0](ids), SHAPES[0][1]), ("tree", SHAPES[3][0](ids), SHAPES[3][1])]
    dq = [_dev_query(ta, q) for q in queries]
    dev = ta.DeviceIndex(segs)
    try:
        with pytest.raises(Exception):  # the default: refused, as for a single segment
            dev.docset(dq)
        dev.set_option("docset_trees", 1)  # (on both segments)
        got = dev.docset(dq)
        for q, g in zip(queries, got):
            w0, w1 = _want(segs[0], q), _want(segs[1], q)
            assert w0.size and w1.size, q
            want = np.concatenate([np.stack([np.zeros_like(w0), w0], axis=1), np.stack([np.ones_like(w1), w1], axis=1)])
            assert g.dtype == np.uint32 and g.shape == want.shape and np.array_equal(g, want), q
        assert np.array_equal(dev.count(dq), np.array([g.shape[0] for g in got], np.uint64))
    finally:
        dev.close()


# ---- 8. scores of these shapes stay refused under either value
def test_scored_stays_refused(ta):
    from tests.test_gpu_docset_scored import _assert_scored, _guard_f32, _ref, _weights

    seg = _synth(60_000, 48)
    good = [(O.MODE_AND, [0, 1]), (O.MODE_OR, [2, 40])]
    want = [_ref(seg, q) for q in good]
    total = sum(w[0].size for w in want)
    phrase = (O.MODE_PHRASE, [0, 1], [0, 1])
    nested = (ta.MODE_BOOL, [1, 2, 3], [M, M, M], [0, 1, 1], 0, {"nested_occurs": [M, M, N]})
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("docset_trees", 1)
        for bad in (phrase, nested):
            for at in (0, 2):
                batch = good[:at] + [bad] + good[at:]
                weights, cache = _weights(seg, batch)
                rc, docs, scores, _ = dev.raw_docset_scored(batch, total + 1000, guard=4, weights=weights, cache=cache)
                assert rc == ERR_UNSUPPORTED, (bad, rc, _err(ta))
                assert ("query %d" % at).encode() in _err(ta), _err(ta)
                assert np.all(docs == GUARD) and np.all(_guard_f32(scores) == GUARD)  # nothing was launched
        weights, cache = _weights(seg, good)
        rc, docs, scores, starts = dev.raw_docset_scored(good, total, weights=weights, cache=cache)
        assert rc == 0, _err(ta)
        _assert_scored(seg, good, docs, scores, starts, want)
        assert dev.last_batch_stats()["kernel_mask"] == ta.binding.KERNEL_DOCSET | ta.binding.KERNEL_DOCSET_SCORE
    finally:
        dev.close()
