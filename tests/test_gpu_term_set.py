"""GPU parity of term sets (tq_term_set_prepare: tantivy_amd/csrc/tq_termset.cpp, tq_termset.hip — what
AutomatonWeight::scorer leaves for FuzzyTermQuery, RegexQuery and TermSetQuery: the OR of N posting lists as a bitset
under a ConstScorer) through tq_count_batch, tq_docset_batch, tq_docset_scored_batch, tq_search_batch and tq_search_one.

Expectations never come from the device: doc sets are numpy unions of the oracle's decode_postings of the members (for
sets of <= 16 members also oracle.bool_match_all of the equivalent clause_of union); scores and top-k rows come from the
literal model of tests/all_model.py, whose `lists` dict takes a set as (present = OR of the members, score =
full(weight)) and whose intersections sort by present.sum(), the reference's cost.  Comparison rule
(tests/test_gpu_docset_scored.py): docs and counts exact; scores bit for bit with at most two scoring lists, within 1e-5
relative otherwise; top-k rows exact (score, doc) sequences with at most two scoring lists."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import all_model as AM
from tests.test_gpu_all import ABSENT_ID, STAR, Lists, T, _same_scores, check_cases
from tests.test_gpu_docset import BOUNDARY_MAX_DOC, ERR_INVALID, ERR_UNSUPPORTED
from tests.test_gpu_round3 import _alive_bytes

pytestmark = pytest.mark.gpu

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
GUARD = 0xDEADBEEF
TERMINATED = 0x7FFFFFFF
KERNEL_TREE, KERNEL_ALL = 0x1000, 0x8000
# the hand-made segment's lists
A, ALL, EVEN, D, ONE, L128, L129, L677 = range(8)
N_EDGE_TERMS = 48


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


def _err(ta):
    return ta.binding.lib().tq_last_error()


@functools.lru_cache(maxsize=None)
def _edge_segment():
    """131 113 docs: 4 098 bitmap words, three 65 536-doc tiles (the rank scan's tile is 2 048 words: two tile borders and a
    partial tile of two words), two tree tiles, a last word of 9 docs.  The four lists of
    tests/test_gpu_docset._boundary_segment, a 1-doc list, lists of exactly 128, of 129 and of 5 x 128 + 37 docs, and 40
    random lists with doc freqs from 2 to 20 000."""
    md = BOUNDARY_MAX_DOC
    rng = np.random.default_rng(20261019)
    a = [31, 32, 33, 63, 64, 65535, 65536, 65537, 131071, 131072, md - 1]
    lists = [a, list(range(md)), list(range(0, md, 2)), list(range(65530, 65545)), [65536]]
    for n in (128, 129, 5 * 128 + 37):
        lists.append(np.sort(rng.choice(md, size=n, replace=False)).tolist())
    dfs = np.unique(np.round(np.geomspace(2, 20_000, N_EDGE_TERMS - len(lists))).astype(int))
    for df in rng.permutation(dfs):
        lists.append(np.sort(rng.choice(md, size=int(df), replace=False)).tolist())
    while len(lists) < N_EDGE_TERMS:  # (rounding made two doc freqs equal)
        lists.append(np.sort(rng.choice(md, size=int(rng.integers(2, 20_000)), replace=False)).tolist())
    tfs = rng.integers(1, 4, size=md)
    norms = rng.integers(1, 40, size=md).tolist()
    return O.build_segment(md, [[(d, int(tfs[d])) for d in l] for l in lists], norms)


@functools.lru_cache(maxsize=None)
def _synth_segment():
    return O.synth_segment(20_000, n_terms=64)


def _union(seg, members):
    """The set's docs: the numpy union of the oracle's decode of every member the segment has."""
    parts = [O.decode_postings(seg, int(t))[0] for t in members if int(t) < len(seg.terms)]
    return np.unique(np.concatenate(parts)).astype(np.uint32) if parts else np.zeros(0, np.uint32)


def _prepare_all_terms(dev, seg):
    """Every term of the segment gets its handle first: a set's handle then lies above every term id (the model's `lists`
    dict is keyed by both)."""
    for t in range(len(seg.terms)):
        dev.term_handle(t)


def _new_set(dev, seg, members):
    h = dev.term_set_prepare(members)
    assert isinstance(h, int) and int(h) >= len(seg.terms), h
    return h


class SetLists(Lists):
    """tests/test_gpu_all.Lists, plus sets: key = the set's handle, present = OR of the members, score = full(weight)."""

    def add_set(self, h, members, weight):
        present = np.zeros(self.seg.max_doc, bool)
        present[_union(self.seg, members)] = True
        self.lists[h] = (present, np.full(self.seg.max_doc, np.float32(weight), np.float32))
        self.weights[h] = float(np.float32(weight))
        return h


def _rows(docs, starts):
    return [docs[int(starts[q]): int(starts[q + 1])] for q in range(len(starts) - 1)]


# ---- 1. the build, at the edges
def _edge_sets(seg, rng):
    by_df = sorted(range(len(seg.terms)), key=lambda t: seg.terms[t].doc_freq)
    big = [t for t in by_df if seg.terms[t].doc_freq >= 2049 and t != ALL]      # a bitmap of their own at dense_ratio 64
    small = [t for t in by_df if 3 <= seg.terms[t].doc_freq < 2049]             # ... none
    return {
        "one member": [ONE],
        "one long member": [EVEN],
        "exactly one block": [L128],
        "a block and a doc": [L129],
        "five blocks and a tail": [L677],
        "bitmap members": big[:6],
        "scattered members": small[:9] + [A, D],
        "mixed": [A, D, L128, L129, L677] + big[-3:] + small[-4:],
        "40 members": [int(t) for t in rng.choice([t for t in range(len(seg.terms)) if t != ALL], size=40, replace=False)],
        "duplicates and absent members": [L677, ABSENT_ID, A, L677, A, ABSENT_ID, big[0], big[0]],
        "empty": [],
        "absent only": [ABSENT_ID, ABSENT_ID],
        "every doc": [ALL, A, L128],
        "every doc from two halves": [EVEN] + big[:2] + [ALL],
    }


@pytest.mark.parametrize("dense_ratio", [1 << 16, 2, 64])
def test_build_at_the_edges(ta, dense_ratio):
    """dense_ratio 65 536: every member of three and more docs has a bitmap (OR-ed word-wise); 2: only the two lists of
    more than half the docs have; 64: mixed.  Every set's doc set, doc count, resident bytes and Count."""
    seg = _edge_segment()
    md = seg.max_doc
    n_words = (md + 31) // 32
    assert n_words == 4098 and md % 32 == 9
    sets = _edge_sets(seg, np.random.default_rng(3))
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", dense_ratio)
        dev.set_option("dense_budget_x", 256)
        _prepare_all_terms(dev, seg)
        n_dense = dev.segment_stats()["n_dense_lists"]
        assert n_dense == sum(1 for t in seg.terms if t.doc_freq * dense_ratio >= md)
        names = list(sets)
        handles = [_new_set(dev, seg, sets[name]) for name in names]
        want = [_union(seg, sets[name]) for name in names]
        assert want[names.index("empty")].size == 0 and want[names.index("absent only")].size == 0
        assert want[names.index("every doc")].size == md and want[names.index("every doc from two halves")].size == md
        assert want[names.index("one member")].tolist() == [65536]
        for name, w in zip(names, want):  # sets of <= 16 members: also the oracle's clause_of union
            members = [t for t in sets[name] if t != ABSENT_ID]
            if 0 < len(members) <= 16:
                d, _ = O.bool_match_all(seg, members, [S] * len(members), [0] * len(members), 0)
                assert np.array_equal(np.asarray(d, np.uint32), w), name
        for h, name, w in zip(handles, names, want):
            assert dev.term_set_info(h) == (w.size, n_words * 8), name
        queries = [(O.MODE_OR, [h]) for h in handles]
        total = sum(w.size for w in want)
        rc, docs, starts = dev.raw_docset(queries, total, guard=8)
        assert rc == 0, _err(ta)
        assert np.all(docs[total:] == GUARD) and int(starts[-1]) == total
        for name, g, w in zip(names, _rows(docs, starts), want):
            assert g.size == w.size and np.array_equal(g, w), (name, dense_ratio, g[:8], w[:8], g.size, w.size)
        cache = np.ones(256, np.float32)
        counts = dev.raw_count([(O.MODE_OR, [h]) for h in handles], [[1.0]] * len(handles), cache)
        assert counts.tolist() == [w.size for w in want]
        assert dev.segment_stats()["n_dense_lists"] == n_dense
    finally:
        dev.close()


# ---- 2. every entry point against the model
def _shape_cases(L, dev, seg, a, b, rare, middle, dense):
    """The issue's shapes over two terms a, b (cost(a) < cost(b)) and sets of chosen costs.  -> (cases with top-k, cases
    without: `* set` is refused by tq_search_batch)."""
    s_r = L.add_set(_new_set(dev, seg, rare), rare, 1.0)
    s_m = L.add_set(_new_set(dev, seg, middle), middle, 1.0)
    s_d = L.add_set(_new_set(dev, seg, dense), dense, 1.0)
    s_w = L.add_set(_new_set(dev, seg, middle), middle, 2.5)
    s_0 = L.add_set(_new_set(dev, seg, middle), middle, 0.0)
    s_e = L.add_set(_new_set(dev, seg, []), [], 1.0)
    for t in (a, b):
        L.need(t)
    cost = lambda key: int(L.lists[key][0].sum())  # noqa: E731
    assert cost(s_r) < cost(a) < cost(s_m) < cost(b) < cost(s_d), [cost(x) for x in (s_r, a, s_m, b, s_d)]
    topk = [
        ([(S, T(s_m))], 0),
        ([(M, T(a)), (M, T(s_m))], 0),
        ([(M, T(a)), (M, T(b)), (M, T(s_r))], 0),
        ([(M, T(a)), (M, T(b)), (M, T(s_m))], 0),
        ([(M, T(a)), (M, T(b)), (M, T(s_d))], 0),
        ([(S, T(a)), (S, T(s_m))], 0),
        ([(M, T(a)), (S, T(s_m))], 0),
        ([(M, T(a)), (N, T(s_m))], 0),
        ([(M, T(s_m)), (N, T(a))], 0),
        ([(S, T(a)), (S, T(b)), (S, T(s_m))], 2),
        ([(M, T(a)), (M, ("union", [b, s_m]))], 0),
        ([(S, T(s_r)), (S, T(s_d))], 0),
        ([(M, T(s_m)), (M, T(s_d))], 0),
        ([(M, T(a)), (M, T(s_w))], 0),
        ([(S, T(s_w))], 0),
        ([(S, T(a)), (S, T(s_0))], 0),
        ([(M, T(s_0))], 0),
        ([(M, T(a)), (M, T(s_e))], 0),
        ([(S, T(a)), (S, T(s_e))], 0),
        ([(M, STAR), (N, T(s_m))], 0),
        ([(M, STAR), (N, T(s_d)), (N, T(a))], 0),
    ]
    no_topk = [([(S, STAR), (S, T(s_m))], 0), ([(S, STAR), (S, T(s_w)), (N, T(a))], 0), ([(M, STAR), (S, T(s_m))], 1)]
    return topk, no_topk


def _spellings(ta, dev, L, cases, alive):
    """TQ_MODE_AND / TQ_MODE_OR spellings of the flat all-Must / all-Should cases: every entry point gives what the
    TQ_MODE_BOOL spelling's model gives."""
    picked = [(c, m) for c, m in cases if m == 0 and all(w[0] == "term" for _, w in c) and len({o for o, _ in c}) == 1 and c[0][0] != N]
    assert len(picked) >= 8
    flat = [(O.MODE_AND if c[0][0] == M else O.MODE_OR, [w[1] for _, w in c]) for c, _ in picked]
    weights = [[L.weights[w[1]] for _, w in c] for c, _ in picked]
    want = [AM.expect(c, 0, L.lists, L.seg.max_doc, alive) for c, _ in picked]
    exact = [len(c) <= 2 for c, _ in picked]
    sizes = [w[0].size for w in want]
    assert dev.raw_count(flat, weights, L.cache).tolist() == sizes
    total = sum(sizes)
    rc, docs, starts = dev.raw_docset(flat, total, guard=2)
    assert rc == 0, _err(ta)
    rc, sdocs, scores, sstarts = dev.raw_docset_scored(flat, total, guard=2, weights=weights, cache=L.cache)
    assert rc == 0, _err(ta)
    assert np.array_equal(starts, sstarts) and np.array_equal(docs[:total], sdocs[:total])
    for i, (g, w) in enumerate(zip(_rows(docs, starts), want)):
        assert np.array_equal(g, w[0]), picked[i]
        assert _same_scores(scores[int(starts[i]): int(starts[i + 1])], w[1], exact[i]), picked[i]
    k = 10
    dev.set_option("record_query_kernels", 1)
    try:
        rows = {}
        for ex in (0, 1):
            sc, dc, ct = dev.raw_search([q + (None,) for q in flat], weights, L.cache, k, opts=(ex, 0))
            rows[ex] = (sc.copy(), dc.copy(), ct.copy())
            # nothing is pruned: the doc-set sizes in both modes, and TQ_KERNEL_TREE whatever the query's mode
            assert dev.last_batch_match_counts(len(flat)).tolist() == sizes, ex
            assert dev.last_batch_query_kernels(len(flat)).tolist() == [KERNEL_TREE] * len(flat), ex
            for i, (wd, ws) in enumerate(want):
                c = int(ct[i])
                assert c == min(k, wd.size), picked[i]
                if exact[i]:
                    es, ed = AM.top_k(wd, ws, k)
                    assert np.array_equal(dc[i, :c], ed) and np.array_equal(sc[i, :c].view(np.uint32), es.view(np.uint32)), picked[i]
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(rows[0], rows[1]))  # every row, bit for bit
    finally:
        dev.set_option("record_query_kernels", 0)
    # tq_search_one: the occurs synthesised on call scratch ride through the submit queue; the batch's row
    sc, dc, ct = rows[0]
    for i, q in enumerate(flat):
        s1, d1, c1 = dev.raw_search_one(q, weights[i], L.cache, k)
        assert c1 == int(ct[i]), (picked[i], c1, int(ct[i]))
        assert np.array_equal(d1[:c1], dc[i, :c1]) and np.array_equal(s1[:c1].view(np.uint32), sc[i, :c1].view(np.uint32)), picked[i]


def _both_modes(ta, dev, L, cases, want, ks):
    """"exhaustive" 0 and 1 give the same rows — every case, bit for bit, not only the ones whose scores the model pins —
    and tq_last_batch_match_counts is the model's doc-set size after either run."""
    from tests.test_gpu_all import _entries, _weights_of

    srch, ws = [], []
    for c, m in cases:
        t, o, cof, whats = _entries(c)
        srch.append((ta.MODE_BOOL, t, None, o, cof, m))
        ws.append(_weights_of(whats, L))
    sizes = [w[0].size for w in want]
    for k in ks:
        rows = []
        for ex in (0, 1):
            sc, dc, ct = dev.raw_search(srch, ws, L.cache, k, opts=(ex, 0))
            rows.append((sc.copy(), dc.copy(), ct.copy()))
            assert dev.last_batch_match_counts(len(srch)).tolist() == sizes, (k, ex)
        for i, case in enumerate(cases):
            for x, y in zip(rows[0], rows[1]):
                assert np.array_equal(x[i].view(np.uint32), y[i].view(np.uint32)), (case, k)


def _search_one_and_kernels(ta, dev, L, cases, rows, alive):
    """tq_search_one gives the batch's row; the queries with a set run as TQ_KERNEL_TREE (`+* -set`: TQ_KERNEL_ALL) and their
    batch mates keep the kernels they have alone."""
    from tests.test_gpu_all import _entries, _weights_of

    k = 10
    sc, dc, ct = rows[(k, 0)]
    for i, (c, m) in enumerate(cases):
        terms, occurs, cof, whats = _entries(c)
        s1, d1, c1 = dev.raw_search_one((ta.MODE_BOOL, terms, occurs, cof, m), _weights_of(whats, L), L.cache, k)
        assert c1 == int(ct[i]), (c, c1, int(ct[i]))
        assert np.array_equal(d1[:c1], dc[i, :c1]) and np.array_equal(s1[:c1].view(np.uint32), sc[i, :c1].view(np.uint32)), c
    terms = sorted(t for t in L.lists if not isinstance(t, ta.binding.RawHandle))[:2]
    mates = [(O.MODE_AND, terms, None), (O.MODE_OR, terms, None), (ta.MODE_BOOL, terms, None, [M, N], None, 0)]
    mate_w = [[L.weights[t] for t in terms]] * 3
    dev.set_option("record_query_kernels", 1)
    try:
        dev.raw_search(mates, mate_w, L.cache, k)
        alone = dev.last_batch_query_kernels(len(mates)).tolist()
        with_set = [c for c in cases if not any(w[0] == "all" for _, w in c[0])][:6]
        with_all = [c for c in cases if any(w[0] == "all" for _, w in c[0])]  # `+* -set`: all_kernel, the set's bits alone
        assert len(with_all) == 2
        srch, ws = [], []
        for c, m in with_set + with_all:
            t, o, cof, whats = _entries(c)
            srch.append((ta.MODE_BOOL, t, None, o, cof, m))
            ws.append(_weights_of(whats, L))
        dev.raw_search(mates[:1] + srch + mates[1:], mate_w[:1] + ws + mate_w[1:], L.cache, k)
        kernels = dev.last_batch_query_kernels(len(mates) + len(srch)).tolist()
        assert kernels[1: 1 + len(srch)] == [KERNEL_TREE] * len(with_set) + [KERNEL_ALL] * len(with_all), kernels
        assert [kernels[0]] + kernels[1 + len(srch):] == alone, (kernels, alone)
        assert KERNEL_TREE not in alone
    finally:
        dev.set_option("record_query_kernels", 0)


@pytest.mark.parametrize("which", ["edge", "synth"])
@pytest.mark.parametrize("with_deletes", [False, True])
def test_every_entry_point_against_the_model(ta, which, with_deletes):
    seg = _edge_segment() if which == "edge" else _synth_segment()
    md = seg.max_doc
    by_df = sorted(range(len(seg.terms)), key=lambda t: seg.terms[t].doc_freq)
    by_df = [t for t in by_df if seg.terms[t].doc_freq < md // 3]  # (the two giant hand-made lists stay out of the shapes)
    n = len(by_df)
    a, b = by_df[n // 2], by_df[-3]
    rare = by_df[2:5] if which == "edge" else by_df[:1]  # (cheaper than a: the Zipf segment's rarest list alone)
    middle = [t for t in by_df[n // 2 - 6: n // 2 + 3] if t != a]
    dense = by_df[-4:]
    alive = None
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        if with_deletes:
            rng = np.random.default_rng(11)
            deleted = rng.choice(md, size=md // 6, replace=False)
            alive = np.ones(md, bool)
            alive[deleted] = False
            dev.set_alive_bitset(_alive_bytes(md, deleted.tolist()))
        L = SetLists(seg)
        topk, no_topk = _shape_cases(L, dev, seg, a, b, rare, middle, dense)
        biggest = max(AM.expect(c, m, L.lists, md, alive)[0].size for c, m in topk if c[0][1] != STAR)
        want, rows = check_cases(ta, dev, L, topk, alive=alive, ks=(10, min(1024, biggest + 7)))
        assert any(w[0].size == 0 for w in want) and any(w[0].size > 10 for w in want)
        _both_modes(ta, dev, L, topk, want, (10, min(1024, biggest + 7)))
        check_cases(ta, dev, L, no_topk, alive=alive, ks=())
        _spellings(ta, dev, L, topk, alive)
        _search_one_and_kernels(ta, dev, L, topk, rows, alive)
    finally:
        dev.close()


# ---- 3. refusals: the code, the query index in the message, and a good call afterwards
def test_refusals_leave_the_segment_usable(ta):
    seg = _synth_segment()
    dev = ta.DeviceIndex([seg])
    lib = ta.binding.lib()
    try:
        _prepare_all_terms(dev, seg)
        members = [3, 9, 20]
        h = _new_set(dev, seg, members)
        want = _union(seg, members)
        cache = np.array(list(O.bm25_for_one_term(1, seg.max_doc, 10.0).cache), np.float32)
        good = (O.MODE_OR, [h])

        def still_good():
            rc, docs, starts = dev.raw_docset([good], want.size)
            assert rc == 0 and np.array_equal(docs[: int(starts[1])], want), _err(ta)
            assert dev.raw_count([good], [[1.0]], cache).tolist() == [want.size]
            sc, dc, ct = dev.raw_search([(O.MODE_OR, [h], None)], [[1.5]], cache, 5)
            assert int(ct[0]) == 5 and dc[0].tolist() == want[:5].tolist() and np.all(sc[0] == np.float32(1.5))

        def refused(fn, code, index, word):
            rc = fn()
            msg = lib.tq_last_error().decode()
            assert rc == code, (rc, msg)
            assert ("query %d" % index) in msg and word in msg, msg
            still_good()

        def rc_of(call):
            def run():
                try:
                    call()
                except ta.TantivyAmdError as e:
                    return e.code
                return 0
            return run

        still_good()
        ok = (O.MODE_AND, [1, 2])
        # a set in a phrase
        phrase = (O.MODE_PHRASE, [1, h], [0, 1])
        refused(lambda: dev.raw_docset([ok, phrase], 1 << 16)[0], ERR_INVALID, 1, "phrase")
        refused(rc_of(lambda: dev.raw_count([ok, ok, (O.MODE_PHRASE, [1, h], [0, 1])], [[1.0, 1.0]] * 3, cache)), ERR_INVALID, 2, "phrase")
        refused(rc_of(lambda: dev.raw_search([(O.MODE_PHRASE, [1, h], [0, 1])], [[1.0, 1.0]], cache, 5)), ERR_INVALID, 0, "phrase")
        nested_phrase = (ta.MODE_BOOL, [1, 2, h], [M, M, M], [0, 1, 1], 0,
                         {"nested_occurs": [M, M | 0x10, M | 0x10], "atom_of": [0, 0, 0], "phrase_offsets": [0, 0, 1]})
        refused(lambda: dev.raw_docset([ok, nested_phrase], 1 << 16)[0], ERR_INVALID, 1, "phrase")
        # nested structure: `+a +(+b +set)`
        nested = (ta.MODE_BOOL, [1, 2, h], [M, M, M], [0, 1, 1], 0, {"nested_occurs": [M, M, M]})
        for option in ("docset_trees", "docset_score_trees"):
            dev.set_option(option, 1)
        refused(lambda: dev.raw_docset([ok, ok, ok, nested], 1 << 16)[0], ERR_UNSUPPORTED, 3, "nested")
        refused(lambda: dev.raw_docset_scored([ok, nested], 1 << 16, weights=[[1.0, 1.0], [1.0] * 3], cache=cache)[0], ERR_UNSUPPORTED, 1, "nested")
        refused(rc_of(lambda: dev.raw_search_trees([nested], [[1.0] * 3], cache, 5)), ERR_UNSUPPORTED, 0, "nested")
        for option in ("docset_trees", "docset_score_trees"):
            dev.set_option(option, 0)
        # `* set` through top-k
        star_set = (ta.MODE_BOOL, [ta.binding.TERM_ALL, h], None, [S, S], None, 0)
        refused(rc_of(lambda: dev.raw_search([(O.MODE_AND, [1, 2], None), star_set], [[1.0, 1.0]] * 2, cache, 5)), ERR_UNSUPPORTED, 1, "match-all")
        # a set as a member of a set; TQ_TERM_ALL as a member
        for bad in ([3, h], [ta.binding.RawHandle(ta.binding.TERM_ALL)], [ta.binding.RawHandle(1 << 30)]):
            with pytest.raises(ta.TantivyAmdError) as e:
                dev.term_set_prepare(bad)
            assert e.value.code == ERR_INVALID, e.value
            still_good()
        # the codec calls
        raw = dev.segment_raw()
        buf = np.zeros(8, np.uint32)
        n_out = ta.binding.C.c_uint64()
        assert lib.tq_decode_postings(raw, int(h), ta.binding._u32(buf), ta.binding._u32(buf)) == ERR_INVALID
        assert b"term set" in lib.tq_last_error()
        assert lib.tq_decode_position_deltas(raw, int(h), ta.binding._u32(buf), 8, ta.binding.C.byref(n_out)) == ERR_INVALID
        still_good()
        # a released handle: in a query, in info, in a second release, as a member
        # (every refusal below is followed by a good call on the same segment: a second set that stays live)
        other_members = [4, 11]
        h_other = _new_set(dev, seg, other_members)
        want_other = _union(seg, other_members)

        def other_still_good():
            rc, docs, starts = dev.raw_docset([(O.MODE_OR, [h_other])], want_other.size)
            assert rc == 0 and np.array_equal(docs[: int(starts[1])], want_other), _err(ta)
            assert dev.raw_count([(O.MODE_AND, [h_other])], [[1.0]], cache).tolist() == [want_other.size]
            sc, dc, ct = dev.raw_search([(O.MODE_OR, [h_other], None)], [[0.5]], cache, 3)
            assert int(ct[0]) == 3 and dc[0].tolist() == want_other[:3].tolist() and np.all(sc[0] == np.float32(0.5))

        other_still_good()
        dev.term_set_release(h)
        for call, index in ((lambda: dev.raw_docset([ok, good], 1 << 16)[0], 1),
                            (rc_of(lambda: dev.raw_count([good], [[1.0]], cache)), 0),
                            (lambda: dev.raw_docset_scored([ok, ok, good], 1 << 16, weights=[[1.0, 1.0]] * 2 + [[1.0]], cache=cache)[0], 2),
                            (rc_of(lambda: dev.raw_search([(O.MODE_OR, [h], None)], [[1.0]], cache, 5)), 0)):
            rc = call()
            msg = lib.tq_last_error().decode()
            assert rc == ERR_INVALID and ("query %d" % index) in msg and "released" in msg, (rc, msg)
            other_still_good()
        for call in (lambda: dev.term_set_info(h), lambda: dev.term_set_release(h), lambda: dev.term_set_prepare([h])):
            with pytest.raises(ta.TantivyAmdError) as e:
                call()
            assert e.value.code == ERR_INVALID, e.value
            other_still_good()
        h = _new_set(dev, seg, members)  # (the slot may be the released one)
        good = (O.MODE_OR, [h])
        still_good()
    finally:
        dev.close()


# ---- 4. lifetime
def test_lifetime_bytes_slots_and_deletes(ta):
    seg = _edge_segment()
    md = seg.max_doc
    set_bytes = (md + 31) // 32 * 8
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        first, second = [A, L129, 20], [D, L677, 33, 41]
        before = dev.segment_stats()
        h1 = _new_set(dev, seg, first)
        mid = dev.segment_stats()
        assert mid["bitmap_bytes"] == before["bitmap_bytes"] + set_bytes == before["bitmap_bytes"] + dev.term_set_info(h1)[1]
        assert mid["n_dense_lists"] == before["n_dense_lists"] and mid["dense_budget_bytes"] == before["dense_budget_bytes"]
        rc, docs, starts = dev.raw_docset([(O.MODE_OR, [h1])], md)
        assert rc == 0 and np.array_equal(docs[: int(starts[1])], _union(seg, first))
        dev.term_set_release(h1)
        after = dev.segment_stats()
        assert after["bitmap_bytes"] == before["bitmap_bytes"] and after["n_dense_lists"] == before["n_dense_lists"]
        h2 = _new_set(dev, seg, second)  # whether or not the slot is reused: the new set's docs
        assert dev.segment_stats()["bitmap_bytes"] == before["bitmap_bytes"] + set_bytes
        rc, docs, starts = dev.raw_docset([(O.MODE_OR, [h2])], md)
        assert rc == 0 and np.array_equal(docs[: int(starts[1])], _union(seg, second))
        assert dev.term_set_info(h2) == (_union(seg, second).size, set_bytes)
        h3 = _new_set(dev, seg, first)  # a third one next to it
        assert int(h3) != int(h2)
        assert dev.segment_stats()["bitmap_bytes"] == before["bitmap_bytes"] + 2 * set_bytes
        # sets prepared before the deletes obey them (the bitmap keeps the deleted docs: info does not change)
        deleted = np.union1d(_union(seg, second)[::2], _union(seg, first)[1::3])
        dev.set_alive_bitset(_alive_bytes(md, deleted.tolist()))
        cache = np.ones(256, np.float32)
        for h, members in ((h2, second), (h3, first)):
            want = np.setdiff1d(_union(seg, members), deleted)
            rc, docs, starts = dev.raw_docset([(O.MODE_OR, [h])], md)
            assert rc == 0 and np.array_equal(docs[: int(starts[1])], want)
            assert dev.raw_count([(O.MODE_OR, [h])], [[1.0]], cache).tolist() == [want.size]
            sc, dc, ct = dev.raw_search([(O.MODE_AND, [h], None)], [[2.0]], cache, 1024, opts=(1, 0))
            assert int(ct[0]) == min(1024, want.size) and np.array_equal(dc[0, : int(ct[0])], want[:1024])
            assert dev.last_batch_match_counts(1).tolist() == [want.size]
            assert dev.term_set_info(h)[0] == _union(seg, members).size
        assert dev.segment_stats()["n_dense_lists"] == before["n_dense_lists"]
    finally:
        dev.close()


def test_timing_leaves_the_build_figures(ta):
    """Option "timing": tq_term_set_prepare leaves the HIP-event time of the build, the HBM model's bytes over what the
    device holds and the number of members it OR-ed word-wise in the batch statistics."""
    seg = _edge_segment()
    md = seg.max_doc
    n_words = (md + 31) // 32
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 64)
        dev.set_option("dense_budget_x", 256)
        _prepare_all_terms(dev, seg)
        dev.set_option("timing", 1)
        cache = np.ones(256, np.float32)
        dev.raw_search([(O.MODE_AND, [EVEN, 33], None)] * 3, [[1.0, 1.0]] * 3, cache, 5)  # (its figures are not read: the build's replace them)
        members = [A, EVEN, L677, 33, 41, 20]
        with_bitmap = [t for t in members if seg.terms[t].doc_freq * 64 >= md]
        assert EVEN in with_bitmap and A not in with_bitmap and L677 not in with_bitmap
        h = _new_set(dev, seg, members)
        st = dev.last_batch_stats()
        scattered = sum(int(seg.terms[t].postings_end - seg.terms[t].postings_start) for t in members if t not in with_bitmap)
        assert st["chunks"] == len(with_bitmap)
        assert st["algorithmic_bytes"] == scattered + 4 * n_words * len(with_bitmap) + 16 * n_words
        assert st["kernel_ms"] > 0.0 and st["batches_averaged"] == 1 and st["matches"] == 0
        assert dev.term_set_info(h)[0] == _union(seg, members).size
    finally:
        dev.close()


# ---- 5. device outputs below the capacity
def test_scored_device_variant_below_capacity(ta):
    import torch

    seg = _synth_segment()
    md = seg.max_doc
    dev = ta.DeviceIndex([seg])
    try:
        _prepare_all_terms(dev, seg)
        L = SetLists(seg)
        members = [5, 17, 40, 41]
        h = L.add_set(_new_set(dev, seg, members), members, 2.5)
        for t in (2, 8):
            L.need(t)
        cases = [([(S, T(h))], 0), ([(M, T(2)), (M, T(h))], 0), ([(S, T(8)), (S, T(h))], 0), ([(M, T(8)), (N, T(h))], 0)]
        queries = [(ta.MODE_BOOL, [w[1] for _, w in c], [o for o, _ in c], None, m) for c, m in cases]
        weights = [[L.weights[w[1]] for _, w in c] for c, _ in cases]
        want = [AM.expect(c, m, L.lists, md) for c, m in cases]
        sizes = [w[0].size for w in want]
        total, n = sum(sizes), len(cases)
        want_starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        cap = total // 2
        assert 0 < cap < total and min(sizes) > 0
        guard32 = int(np.array([GUARD], np.uint32).view(np.int32)[0])
        d_docs = torch.full((total + 64,), guard32, dtype=torch.int32, device="cuda")
        d_scores = torch.full((total + 64,), guard32, dtype=torch.int32, device="cuda").view(torch.float32)
        d_starts = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc = dev.raw_docset_scored_device(queries, d_docs, d_scores, cap, d_starts, weights=weights, cache=L.cache)
        assert rc == 0, _err(ta)
        st = dev.last_batch_stats()  # (waits for the batch)
        torch.cuda.synchronize()
        docs = d_docs.cpu().numpy().view(np.uint32)
        scores = d_scores.cpu().numpy()
        assert np.array_equal(d_starts.cpu().numpy(), want_starts)  # complete, whatever the capacity
        assert np.all(docs[cap:] == GUARD) and np.all(scores[cap:].view(np.uint32) == GUARD)
        assert st["matches"] == total
        for i, (wd, ws) in enumerate(want):
            a = int(want_starts[i])
            keep = max(0, min(cap - a, wd.size))
            assert np.array_equal(docs[a: a + keep], wd[:keep]), cases[i]
            assert _same_scores(scores[a: a + keep], ws[:keep], True), cases[i]
    finally:
        dev.close()


# ---- 6. host mirror: Query::term_set over two segments, scores under the index-wide statistics
def test_host_mirror_over_two_segments(ta):
    segs = [O.synth_segment(5_000, n_terms=32, segment_ord=0), O.synth_segment(3_000, n_terms=32, segment_ord=1)]
    members, a = [3, 9, 20, ABSENT_ID], 5
    SET = ("set", members)
    deleted = [[0, 7, 11, 400], [2999, 5]]
    nd, nt = sum(s.max_doc for s in segs), sum(s.total_num_tokens for s in segs)
    avg = float(np.float32(nt) / np.float32(nd))
    w_a = O.bm25_for_one_term(sum(s.terms[a].doc_freq for s in segs), nd, avg)
    per_seg = []
    for seg, dele in zip(segs, deleted):
        d, s = O.match_all(seg, [a], O.MODE_OR, weights=[w_a])
        pa, sa = np.zeros(seg.max_doc, bool), np.zeros(seg.max_doc, np.float32)
        pa[d], sa[d] = True, s
        ps = np.zeros(seg.max_doc, bool)
        ps[_union(seg, members)] = True
        alive = np.ones(seg.max_doc, bool)
        alive[dele] = False
        per_seg.append((pa, sa, ps, alive))
    # (host tuple, model clauses, the set's boost)
    cases = [((O.MODE_OR, [SET], {"boosts": [2.5]}), [(S, T("set"))], 2.5),
             ((O.MODE_AND, [a, SET]), [(M, T(a)), (M, T("set"))], 1.0),
             ((ta.MODE_BOOL, [a, SET], [M, S], None, 0, {"boosts": [1.0, 0.5]}), [(M, T(a)), (S, T("set"))], 0.5),
             ((ta.MODE_BOOL, [a, SET], [M, N]), [(M, T(a)), (N, T("set"))], 1.0),
             ((ta.MODE_BOOL, [SET, a], [S, S], None, 2), [(S, T("set")), (S, T(a))], 1.0)]
    want = []
    for _, clauses, boost in cases:
        rows = []
        for o, (pa, sa, ps, alive) in enumerate(per_seg):
            lists = {a: (pa, sa), "set": (ps, np.full(ps.size, np.float32(boost), np.float32))}
            minimum = 2 if len(clauses) == 2 and clauses[0][0] == S and clauses[1][0] == S else 0
            d, s = AM.expect(clauses, minimum, lists, ps.size, alive)
            rows += [(o, int(x), np.float32(y)) for x, y in zip(d, s)]
        want.append(rows)
    assert all(len(w) > 10 for w in want)
    queries = [c[0] for c in cases]
    dev = ta.DeviceIndex(segs)
    try:
        for o in range(2):
            dev.set_alive_bitset(_alive_bytes(segs[o].max_doc, deleted[o]), segment_ord=o)
        assert dev.count(queries).tolist() == [len(w) for w in want]
        for rows, w in zip(dev.docset(queries), want):
            assert [tuple(r) for r in rows.tolist()] == [(o, d) for o, d, _ in w]
        for (pairs, scores), w in zip(dev.docset_scored(queries), want):
            assert [tuple(r) for r in pairs.tolist()] == [(o, d) for o, d, _ in w]
            assert np.array_equal(scores.view(np.uint32), np.array([s for _, _, s in w], np.float32).view(np.uint32))
        sc, ords, docs, ct = dev.search(queries, 10)
        for i, w in enumerate(want):  # merge_top_k: (score desc, segment asc, doc asc)
            top = sorted(w, key=lambda r: (-float(r[2]), r[0], r[1]))[:10]
            assert int(ct[i]) == 10, cases[i][0]
            assert list(zip(ords[i].tolist(), docs[i].tolist())) == [(o, d) for o, d, _ in top], cases[i][0]
            assert np.array_equal(sc[i].view(np.uint32), np.array([s for _, _, s in top], np.float32).view(np.uint32)), cases[i][0]
        # the sets live as long as the prepared Weights: each segment holds one table per set of the batch
        set_bytes = [(s.max_doc + 31) // 32 * 8 for s in segs]
        before = [dev.segment_stats(o)["bitmap_bytes"] for o in range(2)]
        dev.prepare([(O.MODE_OR, [a])])  # the batch with the sets is replaced: they are released
        after = [dev.segment_stats(o)["bitmap_bytes"] for o in range(2)]
        assert [b - x for b, x in zip(before, after)] == [len(cases) * sb for sb in set_bytes]
        # deeper than a direct clause: Unsupported
        with pytest.raises(ta.TantivyAmdError) as e:
            dev.search([(ta.MODE_BOOL, [a, SET, 6], [M, M, M], [0, 1, 1], 0, {"nested_occurs": [255, 1, 1]})], 5)
        assert e.value.code == ERR_UNSUPPORTED
        assert dev.count(queries[:2]).tolist() == [len(w) for w in want[:2]]  # live Weights with sets: closed below
    finally:
        dev.close()
    dev = ta.DeviceIndex(segs)  # closing the index with live Weights left the process and the device usable
    try:
        assert dev.count(queries[:1]).tolist() == [sum(int(ps.sum()) for _, _, ps, _ in per_seg)]
    finally:
        dev.close()
