"""GPU parity of AllQuery clauses (TQ_TERM_ALL: tantivy_amd/csrc/tq_all.cpp, tq_all.hip, and the count / doc-set paths)
through tq_search_batch, tq_search_one, tq_count_batch, tq_docset_batch and tq_docset_scored_batch.

Every expectation comes from the literal model of BooleanWeight::complex_scorer in tests/all_model.py, fed with per-term
(docs, scores) from the oracle's match_all — never from the device.  Comparison rule (tests/test_gpu_docset_scored.py):
docs and counts exact; scores bit for bit for queries with at most two scoring lists, within 1e-5 relative otherwise;
top-k rows of queries with at most two scoring lists are exact (score, doc) sequences."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import all_model as AM
from tests.helpers import corpus_segment
from tests.test_gpu_docset import BOUNDARY_MAX_DOC, ERR_INVALID, ERR_UNSUPPORTED, _boundary_segment
from tests.test_gpu_round3 import _alive_bytes

pytestmark = pytest.mark.gpu

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
STAR = ("all", 1.0)
NONE = ("absent",)
ABSENT_ID = 1_000_000  # a term id no segment of these tests has
TERMINATED = 0x7FFFFFFF


def T(t):
    return ("term", t)


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


def _err(ta):
    return ta.binding.lib().tq_last_error()


class Lists:
    """Per-term dense (present, score) arrays of a segment from the oracle's match_all, and the f32 weights behind them."""

    def __init__(self, seg, boosts=None):
        self.seg, self.boosts, self.lists, self.weights = seg, boosts or {}, {}, {}
        self.avg = float(np.float32(seg.total_num_tokens) / np.float32(seg.max_doc))
        self.cache = np.array(list(O.bm25_for_one_term(1, seg.max_doc, self.avg).cache), np.float32)

    def need(self, t):
        if t in self.lists or t >= len(self.seg.terms):
            return
        w = O.bm25_for_one_term(self.seg.terms[t].doc_freq, self.seg.max_doc, self.avg, self.boosts.get(t, 1.0))
        d, s = O.match_all(self.seg, [t], O.MODE_OR, weights=[w])
        present = np.zeros(self.seg.max_doc, bool)
        score = np.zeros(self.seg.max_doc, np.float32)
        present[d] = True
        score[d] = s
        self.lists[t], self.weights[t] = (present, score), float(w.weight)


def _entries(clauses):
    """The clauses (one entry each, or a ("union", [terms]) clause) as parallel entry lists."""
    terms, occurs, cof, whats = [], [], [], []
    for c, (occur, what) in enumerate(clauses):
        for w in ([T(t) for t in what[1]] if what[0] == "union" else [what]):
            terms.append(ta_all() if w[0] == "all" else ABSENT_ID if w[0] == "absent" else w[1])
            occurs.append(occur)
            cof.append(c)
            whats.append(w)
    return terms, occurs, cof, whats


def ta_all():
    return 0xFFFFFFFE  # binding.TERM_ALL


def _model_clauses(clauses, L):
    """Absent term ids become ("absent",) for the model; the lists it needs are fetched from the oracle."""
    out = []
    for occur, what in clauses:
        if what[0] == "term":
            L.need(what[1])
            what = what if what[1] in L.lists else NONE
        elif what[0] == "union":
            for t in what[1]:
                L.need(t)
        out.append((occur, what))
    return out


def _n_scoring(clauses, L):
    n = 0
    for occur, what in clauses:
        if occur == N:
            continue
        n += sum(1 for t in (what[1] if what[0] == "union" else [what[1]] if what[0] == "term" else []) if t in L.lists)
    return n


def _weights_of(whats, L):
    return [float(w[1]) if w[0] == "all" else L.weights.get(w[1], 1.0) if w[0] == "term" else 1.0 for w in whats]


def _flat(ta, clauses, minimum):
    terms, occurs, cof, _ = _entries(clauses)
    return (ta.MODE_BOOL, terms, occurs, cof, minimum)


def _searchq(ta, clauses, minimum):
    terms, occurs, cof, _ = _entries(clauses)
    return (ta.MODE_BOOL, terms, None, occurs, cof, minimum)


def _same_scores(got, want, exact):
    if exact:
        return np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return np.allclose(got, want, rtol=1e-5, atol=0)


def check_cases(ta, dev, L, cases, alive=None, ks=(10,), exhaustive=(0, 1)):
    """cases = [(clauses, minimum)].  All four entry points against the literal model."""
    model = [_model_clauses(c, L) for c, _ in cases]
    want = [AM.expect(mc, m, L.lists, L.seg.max_doc, alive) for mc, (_, m) in zip(model, cases)]
    exact = [_n_scoring(mc, L) <= 2 for mc in model]
    weights = [_weights_of(_entries(c)[3], L) for c, _ in cases]
    flat = [_flat(ta, c, m) for c, m in cases]
    srch = [_searchq(ta, c, m) for c, m in cases]
    n = len(cases)
    sizes = [w[0].size for w in want]
    # Count
    counts = dev.raw_count(srch, weights, L.cache)
    assert counts.tolist() == sizes, [(cases[i], int(counts[i]), sizes[i]) for i in range(n) if counts[i] != sizes[i]][:3]
    # doc sets, with and without scores
    total = sum(sizes)
    rc, docs, starts = dev.raw_docset(flat, total, guard=4)
    assert rc == 0, _err(ta)
    assert np.diff(starts.astype(np.int64)).tolist() == sizes
    rc, sdocs, scores, sstarts = dev.raw_docset_scored(flat, total, guard=4, weights=weights, cache=L.cache)
    assert rc == 0, _err(ta)
    assert np.array_equal(sstarts, starts) and np.array_equal(sdocs[:total], docs[:total])
    assert np.all(docs[total:] == 0xDEADBEEF) and np.all(sdocs[total:] == 0xDEADBEEF)
    for i in range(n):
        a, b = int(starts[i]), int(starts[i + 1])
        assert np.array_equal(docs[a:b], want[i][0]), (cases[i], docs[a:b][:8], want[i][0][:8])
        assert _same_scores(scores[a:b], want[i][1], exact[i]), (cases[i], scores[a:b][:4], want[i][1][:4])
    # top-k
    rows = {}
    for k in ks:
        for ex in exhaustive:
            sc, dc, ct = dev.raw_search(srch, weights, L.cache, k, opts=(ex, 0))
            rows[(k, ex)] = (sc.copy(), dc.copy(), ct.copy())
            if ex:
                assert dev.last_batch_match_counts(n).tolist() == sizes
            for i in range(n):
                wd, ws = want[i]
                c = int(ct[i])
                assert c == min(k, wd.size), (cases[i], k, ex, c, wd.size)
                assert np.all(sc[i, c:] == 0.0) and np.all(dc[i, c:] == TERMINATED), (cases[i], k)
                if exact[i]:
                    es, ed = AM.top_k(wd, ws, k)
                    assert np.array_equal(dc[i, :c], ed), (cases[i], k, ex, dc[i, :c][:8], ed[:8])
                    assert np.array_equal(sc[i, :c].view(np.uint32), es.view(np.uint32)), (cases[i], k, ex)
                else:  # 3+ lists: every returned doc is in the set with its own score, and no better doc is missing
                    pos = np.searchsorted(wd, dc[i, :c])
                    assert np.all(pos < wd.size) and np.array_equal(wd[np.minimum(pos, wd.size - 1)], dc[i, :c]), cases[i]
                    assert np.allclose(sc[i, :c], ws[pos], rtol=1e-5, atol=0), cases[i]
                    if c:
                        last = float(sc[i, c - 1])
                        missing = np.setdiff1d(np.nonzero(ws > last + abs(last) * 1e-5)[0], pos)
                        assert missing.size == 0, (cases[i], k, wd[missing][:4])
        lo, hi = rows[(k, exhaustive[0])], rows[(k, exhaustive[-1])]  # "exhaustive" 0 and 1: the same rows
        assert all(np.array_equal(x[i], y[i]) for x, y in zip(lo, hi) for i in range(n) if exact[i]), k
    return want, rows


# ---- 1. the reference's own tests
def test_reference_kats(ta):
    """boolean_query/mod.rs:383-418 (`* * a a a` with minimum 4 counts 1), :444-548 (`* hello`, `hello *` count 6;
    `+* apple` counts 4), :361-369 (`* none` is the AllScorer)."""
    seg2, v2 = corpus_segment(["apple", "banana"])
    seg6, v6 = corpus_segment(["hello", "world", "hello world", "foo", "bar", "baz"])
    seg4, v4 = corpus_segment(["apple", "banana", "cherry", "date"])
    for seg, cases, sizes in (
            (seg2, [([(S, STAR), (S, STAR)] + [(S, T(v2["apple"]))] * 3, 4)], [1]),
            (seg6, [([(S, STAR), (S, T(v6["hello"]))], 0), ([(S, T(v6["hello"])), (S, STAR)], 0), ([(S, STAR), (S, NONE)], 0)],
             [6, 6, 6]),
            (seg4, [([(M, STAR), (S, T(v4["apple"]))], 0)], [4])):
        dev = ta.DeviceIndex([seg])
        try:
            want, _ = check_cases(ta, dev, Lists(seg), cases, ks=(3, 10))
            assert [w[0].size for w in want] == sizes
        finally:
            dev.close()


# ---- 2. `*` alone
@functools.lru_cache(maxsize=None)
def _tiny_segment(md):
    return O.build_segment(md, [[(0, 1)]], [3] * md)


@pytest.mark.parametrize("md", [1, 9, 31, 32, 33, BOUNDARY_MAX_DOC])
def test_star_alone(ta, md):
    seg = _boundary_segment()[0] if md == BOUNDARY_MAX_DOC else _tiny_segment(md)
    assert seg.max_doc == md
    deleted = sorted({d for d in (0, 31, 32, 65535, 65536, md - 1) if d < md})
    for dele in ([], deleted):
        alive = np.ones(md, bool)
        alive[dele] = False
        first = np.nonzero(alive)[0].astype(np.uint32)
        dev = ta.DeviceIndex([seg])
        try:
            if dele:
                dev.set_alive_bitset(_alive_bytes(md, dele))
            L = Lists(seg)
            cases = [([(S, STAR)], 0), ([(M, STAR)], 0), ([(S, ("all", 2.5))], 0), ([(M, ("all", -1.0))], 0)]
            want, rows = check_cases(ta, dev, L, cases, alive=alive, ks=(1, 10, 200))
            for (k, _), (sc, dc, ct) in rows.items():
                c = min(k, first.size)
                assert ct.tolist() == [c] * 4
                for i, base in enumerate((1.0, 1.0, 2.5, -1.0)):
                    assert np.array_equal(dc[i, :c], first[:c]) and np.all(sc[i, :c] == np.float32(base))
            assert all(w[0].size == first.size for w in want)
            # a batch of `*` alone counts without a kernel
            assert dev.raw_count([(ta.MODE_OR, [ta.binding.TERM_ALL])], [[1.0]], L.cache).tolist() == [first.size]
            assert dev.last_batch_stats()["kernel_mask"] == 0
            # mode AND / OR spellings, and the kernel family of the top-k
            sc, dc, ct = dev.raw_search([(ta.MODE_AND, [ta.binding.TERM_ALL]), (ta.MODE_OR, [ta.binding.TERM_ALL])],
                                        [[1.0], [1.0]], L.cache, 10)
            assert ct.tolist() == [min(10, first.size)] * 2 and np.array_equal(dc[0], dc[1])
            assert dev.last_batch_stats()["kernel_mask"] == ta.binding.KERNEL_ALL
        finally:
            dev.close()


# ---- 3. exclusion at the word, tile and segment boundaries
@pytest.mark.parametrize("dense_ratio", [4096, 2, 1 << 16])
def test_exclusion_at_boundaries(ta, dense_ratio):
    seg, _ = _boundary_segment()
    A, B, Cc, D = 0, 1, 2, 3
    cases = [([(M, STAR), (N, T(Cc))], 0), ([(S, STAR), (N, T(Cc)), (N, T(D))], 0), ([(M, STAR), (N, T(B))], 0),
             ([(N, STAR)], 0), ([(M, T(A)), (N, STAR)], 0), ([(M, STAR), (S, T(A)), (N, T(D))], 0),
             ([(M, STAR), (S, T(A)), (S, T(D))], 1)]
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", dense_ratio)
        dev.set_option("dense_budget_x", 256)
        want, _ = check_cases(ta, dev, Lists(seg), cases, ks=(10, 300))
        md = seg.max_doc
        odd = np.arange(1, md, 2, dtype=np.uint32)
        assert np.array_equal(want[0][0], odd) and want[2][0].size == 0 and want[3][0].size == 0 and want[4][0].size == 0
        assert np.array_equal(want[1][0], odd[(odd < 65530) | (odd >= 65545)])
    finally:
        dev.close()


# ---- 4. score shapes
@functools.lru_cache(maxsize=None)
def _synth():
    return O.synth_segment(20_000, n_terms=64)


def _shape_cases(a, b, c):
    return [([(M, STAR), (S, T(a))], 0), ([(S, STAR), (S, T(a))], 0), ([(M, STAR), (S, T(a)), (S, T(b))], 0),
            ([(S, STAR), (S, T(a)), (S, T(b))], 0), ([(S, STAR), (S, T(a)), (S, T(b))], 1),
            ([(M, STAR), (S, T(a)), (S, T(b))], 2),               # a + b, no + 1
            ([(M, STAR), (S, T(a)), (S, T(b)), (S, T(c))], 2),    # at least two of three, s + 1
            ([(S, STAR), (S, STAR), (S, T(a))], 2),               # every doc, s + 1
            ([(M, STAR), (S, STAR)], 0),
            ([(M, STAR), (M, T(a))], 0), ([(M, T(a)), (S, STAR)], 0),  # PLAIN
            ([(M, STAR), (S, T(a)), (N, T(b))], 0),
            ([(M, STAR), (S, ("union", [a, b])), (S, T(c))], 0),
            ([(M, STAR), (S, ("union", [a, b])), (S, T(c))], 1),
            ([(S, STAR), (S, NONE), (S, T(a))], 0), ([(M, STAR), (S, NONE)], 1)]


def test_score_shapes(ta):
    seg = _synth()
    dfs = sorted(range(len(seg.terms)), key=lambda t: seg.terms[t].doc_freq)
    # the rarest lists (150-155 postings, no bitmap of their own at the default "dense_ratio": the probe pool) — k = 300
    # exceeds the size of `a` alone, so base-only docs fill the tail of `+* a` in doc order; the second pass takes the
    # most frequent lists (bitmaps of their own)
    rare = dfs[:3]
    assert seg.terms[rare[0]].doc_freq < 300
    common = dfs[-3:]
    dev = ta.DeviceIndex([seg])
    try:
        for a, b, c in (rare, common):
            L = Lists(seg)
            cases = _shape_cases(a, b, c)
            want, rows = check_cases(ta, dev, L, cases, ks=(10, 300))
            assert dev.last_batch_stats()["kernel_mask"] & ta.binding.KERNEL_ALL
            # `+* +a` and `+a *` are the query without the All, bit for bit
            plain_s, plain_d, plain_c = dev.raw_search([_searchq(ta, [(M, T(a))], 0)], [[L.weights[a]]], L.cache, 300,
                                                       opts=(1, 0))
            for i in (9, 10):
                sc, dc, ct = rows[(300, 1)]
                assert ct[i] == plain_c[0] and np.array_equal(dc[i], plain_d[0])
                assert np.array_equal(sc[i].view(np.uint32), plain_s[0].view(np.uint32))
            if [a, b, c] == rare:  # `+* a`, k = 300: the docs of a first, then base-only docs in doc order
                sc, dc, ct = rows[(300, 0)]
                held = np.nonzero(L.lists[a][0])[0]
                assert held.size < 300 and ct[0] == 300
                tail = dc[0, held.size:]
                assert np.all(sc[0, held.size:] == np.float32(1.0)) and np.all(sc[0, : held.size] > np.float32(1.0))
                assert np.array_equal(tail, np.setdiff1d(np.arange(seg.max_doc), held)[: 300 - held.size])
        # negative Should weights: s + 1 < 1 for some docs, which then rank below the docs that hold no list
        a, b, c = common
        L = Lists(seg, boosts={a: -1.0, b: -0.5})
        want, rows = check_cases(ta, dev, L, _shape_cases(a, b, c)[:5] + _shape_cases(a, b, c)[11:12], ks=(10, 300))
        assert np.any(want[0][1] < 1.0) and np.any(want[0][1] == 1.0)
    finally:
        dev.close()


# ---- 5. a mixed batch
def test_mixed_batch(ta):
    seg = O.synth_segment(20_000, n_terms=64, with_positions=True)
    L = Lists(seg)
    B = ta.binding
    for t in range(8):
        L.need(t)
    w = lambda ts: [L.weights[t] for t in ts]  # noqa: E731
    ordinary = [(O.MODE_AND, [0, 1]), (O.MODE_OR, [2, 3]), (O.MODE_PHRASE, [0, 1], [0, 1]),
                (ta.MODE_BOOL, [4, 5, 6], None, [M, S, N], None, 0)]
    ow = [w([0, 1]), w([2, 3]), [L.weights[0] + L.weights[1]], w([4, 5, 6])]
    alls = [(_searchq(ta, [(M, STAR), (S, T(7))], 0), [1.0, L.weights[7]], True),     # ALL-BASED
            (_searchq(ta, [(M, STAR), (M, T(7))], 0), [1.0, L.weights[7]], False),    # PLAIN
            (_searchq(ta, [(S, STAR), (N, T(2))], 0), [1.0, L.weights[2]], True),
            (_searchq(ta, [(N, STAR), (S, T(2))], 0), [1.0, L.weights[2]], False)]    # EMPTY
    queries, weights, is_all = [], [], []
    for i in range(4):
        queries += [ordinary[i], alls[i][0]]
        weights += [ow[i], alls[i][1]]
        is_all += [False, alls[i][2]]
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("record_query_kernels", 1)
        base = dev.raw_search(ordinary, ow, L.cache, 10)
        sc, dc, ct = dev.raw_search(queries, weights, L.cache, 10)
        st = dev.last_batch_stats()
        assert st["kernel_mask"] & B.KERNEL_ALL
        kern = dev.last_batch_query_kernels(len(queries))
        assert [bool(k & B.KERNEL_ALL) for k in kern] == is_all
        for i in range(4):
            assert ct[2 * i] == base[2][i] and np.array_equal(dc[2 * i], base[1][i])
            assert np.array_equal(sc[2 * i].view(np.uint32), base[0][i].view(np.uint32))
        assert ct[7] == 0
        # the All rows against the model
        for j, (clauses, m) in ((1, ([(M, STAR), (S, T(7))], 0)), (3, ([(M, STAR), (M, T(7))], 0)),
                                (5, ([(S, STAR), (N, T(2))], 0))):
            wd, ws = AM.expect(_model_clauses(clauses, L), m, L.lists, seg.max_doc)
            es, ed = AM.top_k(wd, ws, 10)
            assert np.array_equal(dc[j, : ct[j]], ed) and np.array_equal(sc[j, : ct[j]].view(np.uint32), es.view(np.uint32))
        # one All query through tq_search_one
        s1, d1, c1 = dev.raw_search_one(_flat(ta, [(M, STAR), (S, T(7))], 0), [1.0, L.weights[7]], L.cache, 10)
        assert c1 == ct[1] and np.array_equal(d1, dc[1]) and np.array_equal(s1.view(np.uint32), sc[1].view(np.uint32))
    finally:
        dev.close()


# ---- 6. refusals
def test_refusals_leave_the_segment_usable(ta):
    seg = _synth()
    L = Lists(seg)
    L.need(3)
    L.need(4)
    B = ta.binding
    ALL = B.TERM_ALL
    dev = ta.DeviceIndex([seg])

    def still_works():
        sc, dc, ct = dev.raw_search([(O.MODE_OR, [3])], [[L.weights[3]]], L.cache, 5)
        wd, ws = AM.expect([(S, T(3))], 0, L.lists, seg.max_doc)
        assert np.array_equal(dc[0, : ct[0]], AM.top_k(wd, ws, 5)[1])

    try:
        w2 = [2.0, L.weights[3]]
        boosted = (ta.MODE_BOOL, [ALL, 3], None, [M, S], None, 0)
        with pytest.raises(B.TantivyAmdError) as e:  # a boosted All beside a term: scores stay on the CPU
            dev.raw_search([(O.MODE_OR, [4]), boosted], [[L.weights[4]], w2], L.cache, 5)
        assert e.value.code == ERR_UNSUPPORTED and "query 1" in str(e.value)
        still_works()
        flat = (ta.MODE_BOOL, [ALL, 3], [M, S], None, 0)
        rc, _, _, _ = dev.raw_docset_scored([(O.MODE_OR, [4]), flat], 2 * seg.max_doc, weights=[[L.weights[4]], w2], cache=L.cache)
        assert rc == ERR_UNSUPPORTED and b"query 1" in _err(ta)
        still_works()
        # ... while count and docset take it, with the doc set the boost does not change
        assert dev.raw_count([boosted], [w2], L.cache).tolist() == [seg.max_doc]
        rc, docs, starts = dev.raw_docset([flat], seg.max_doc)
        assert rc == 0 and int(starts[1]) == seg.max_doc and np.array_equal(docs, np.arange(seg.max_doc, dtype=np.uint32))
        # All in a phrase
        with pytest.raises(B.TantivyAmdError) as e:
            dev.raw_search([(O.MODE_PHRASE, [ALL, 3], [0, 1])], [[1.0, 1.0]], L.cache, 5)
        assert e.value.code == ERR_INVALID
        still_works()
        # All sharing a clause_of value; All in a nested tree
        for q in ((ta.MODE_BOOL, [ALL, 3, 4], [S, S, S], [0, 0, 1], 0),
                  (ta.MODE_BOOL, [4, ALL, 3], [M, M, M], [0, 1, 1], 0, {"nested_occurs": [255, 1, 1]})):
            rc, _, _ = dev.raw_docset([q], seg.max_doc)
            assert rc == ERR_UNSUPPORTED and b"query 0" in _err(ta), (q, _err(ta))
            still_works()
        with pytest.raises(B.TantivyAmdError) as e:
            dev.raw_search([(ta.MODE_BOOL, [ALL, 3, 4], None, [S, S, S], [0, 0, 1], 0)], [[1.0, 1.0, 1.0]], L.cache, 5)
        assert e.value.code == ERR_UNSUPPORTED
        with pytest.raises(B.TantivyAmdError) as e:
            dev.raw_count([(ta.MODE_BOOL, [ALL, 3, 4], None, [S, S, S], [0, 0, 1], 0)], [[1.0, 1.0, 1.0]], L.cache)
        assert e.value.code == ERR_UNSUPPORTED
        with pytest.raises(B.TantivyAmdError) as e:  # a boost that is not finite
            dev.raw_search([(O.MODE_OR, [ALL])], [[float("inf")]], L.cache, 5)
        assert e.value.code == ERR_INVALID
        still_works()
    finally:
        dev.close()


# ---- 7. the host mirror over two segments
def test_host_mirror(ta):
    segs = [O.synth_segment(5_000, n_terms=32, segment_ord=0), O.synth_segment(3_000, n_terms=32, segment_ord=1)]
    B = ta.binding
    ALL = B.TERM_ALL
    deleted = [[0, 7], [2999]]
    dev = ta.DeviceIndex(segs)
    try:
        for o in range(2):
            dev.set_alive_bitset(_alive_bytes(segs[o].max_doc, deleted[o]), segment_ord=o)
        alive = [np.setdiff1d(np.arange(s.max_doc), d) for s, d in zip(segs, deleted)]
        n_alive = sum(a.size for a in alive)
        # Query::all() top-5: the first five alive docs of segment 0 (ties go to the lower segment ordinal)
        sc, ords, docs, ct = dev.search([(ta.MODE_OR, [ALL])], 5)
        assert ct[0] == 5 and ords[0].tolist() == [0] * 5 and docs[0].tolist() == alive[0][:5].tolist()
        assert np.all(sc[0] == np.float32(1.0))
        sc, ords, docs, ct = dev.search([(ta.MODE_OR, [ALL], {"boosts": [2.5]})], 5)
        assert np.all(sc[0] == np.float32(2.5)) and docs[0].tolist() == alive[0][:5].tolist()
        # one-clause BooleanQuery of AllQuery with minimum 3 still matches everything (boolean_weight.rs:463-469)
        one = (ta.MODE_BOOL, [ALL], [S], None, 3)
        assert dev.count([(ta.MODE_OR, [ALL]), one, (ta.MODE_BOOL, [ALL], [N])]).tolist() == [n_alive, n_alive, 0]
        # `+* -a`: ordered by (segment, doc)
        a = 5
        rows = dev.docset([(ta.MODE_BOOL, [ALL, a], [M, N])])[0]
        want = []
        for o, seg in enumerate(segs):
            d, _ = O.match_all(seg, [a], O.MODE_OR)
            want += [(o, int(x)) for x in np.setdiff1d(alive[o], d)]
        assert [tuple(r) for r in rows.tolist()] == want
        pairs, scores = dev.docset_scored([(ta.MODE_BOOL, [ALL, a], [M, N])])[0]
        assert [tuple(r) for r in pairs.tolist()] == want and np.all(scores == np.float32(1.0))
        # an All inside a nested BooleanQuery stays on the CPU
        with pytest.raises(B.TantivyAmdError) as e:
            dev.search([(ta.MODE_BOOL, [a, ALL, 6], [M, M, M], [0, 1, 1], 0, {"nested_occurs": [255, 1, 1]})], 5)
        assert e.value.code == ERR_UNSUPPORTED
    finally:
        dev.close()


# ---- 8. fuzz
def test_fuzz(ta):
    """300 random flat queries with random All insertion under a seeded random alive bitset, all four entry points.
    Shapes the device refuses (a boosted All beside other clauses, All inside unions) are not generated; every
    generated query is checked."""
    seg = _synth()
    rng = np.random.default_rng(8)
    dele = np.sort(rng.choice(seg.max_doc, size=700, replace=False)).tolist()
    alive = np.ones(seg.max_doc, bool)
    alive[dele] = False
    cases = []
    while len(cases) < 300:
        n = int(rng.integers(1, 6))
        terms = rng.choice(64, size=n, replace=False).tolist()
        clauses = []
        for t in terms:
            occur = int(rng.choice([S, S, M, N]))
            r = rng.random()
            clauses.append((occur, STAR if r < 0.3 else NONE if r < 0.36 else T(int(t))))
        if rng.random() < 0.5:
            clauses.insert(int(rng.integers(0, len(clauses) + 1)), (int(rng.choice([S, M])), STAR))
        minimum = int(rng.integers(0, 4)) if len(clauses) > 1 else 0
        cases.append((clauses, minimum))
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_alive_bitset(_alive_bytes(seg.max_doc, dele))
        L = Lists(seg)
        check_cases(ta, dev, L, cases, alive=alive, ks=(10,))
    finally:
        dev.close()
