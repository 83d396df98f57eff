"""PhraseQuery with slop > 0 on the device (tantivy_amd/csrc/tq_phrase_slop.hip, TQ_KERNEL_PHRASE_SLOP) against the
plain model of tests/slop_model.py, which tests/test_slop_model_cpu.py pins to the reference's own vectors.  The model is
the reference in every comparison, never another device path.  Doc sets, counts and hit counts are exact; a score is
compared by the criterion of tests/test_gpu_phrase_positions.py (_assert_model: within 1e-5 of the model's float64
score, which pins the phrase count).

Scoring entry points (search, device rows, search_one) take the COUNTING verdict, tq_count_batch and doc sets the
EXISTENCE verdict: the two differ for three and more terms, as in the reference.

The planted corpus S is a few thousand postings in a segment of 132 585 docs: a tile of the kernel is
TQK_TREE_TILE_WORDS = 4 096 words = 131 072 docs, and matches on both sides of that boundary need that many doc ids."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import phrase_model as PM
from tests import slop_model as SM
from tantivy_amd.binding import SLOP_CARRY_CAP as CAP  # TQ_SLOP_CARRY_CAP (tests/test_abi_slop_cpu.py: = the header's)
from tests.test_gpu_phrase_positions import K_ALL, _assert_model, _open, _rows, ta  # noqa: F401  (ta: the fixture)

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = 1, 4
TILE_DOCS = 4096 * 32


def _err(ta):
    return ta.binding.lib().tq_last_error().decode()


def _q(terms, offs, slop):
    return (O.MODE_PHRASE, list(terms), list(offs), int(slop))


@functools.lru_cache(maxsize=None)
def _expect(corp, qi, slop):
    _, terms, offs = corp.queries[qi]
    return SM.SlopExpect(corp.tp, terms, offs, slop, corp.fieldnorms, corp.alive)


def _check_scored(ta, dev, corp, picked, slop, k=K_ALL):
    """One search batch of the queries `picked` at `slop`: rows, match counts, kernel family, overflow words."""
    B = ta.binding
    queries = [_q(corp.queries[qi][1], corp.queries[qi][2], slop) for qi in picked]
    full = _rows(dev.search(queries, k), len(queries))
    kern = dev.last_batch_query_kernels(len(queries))
    counts = dev.last_batch_match_counts(len(queries))
    over = dev.last_batch_slop_overflows(len(queries))
    assert dev.last_batch_stats()["kernel_mask"] == B.KERNEL_PHRASE_SLOP
    for at, qi in enumerate(picked):
        e = _expect(corp, qi, slop)
        _assert_model(corp, "%s~%d" % (corp.queries[qi][0], slop), full[at][0], full[at][1], e.docs, e.scores)
        assert int(counts[at]) == e.docs.size and int(over[at]) == 0
        assert int(kern[at]) == B.KERNEL_PHRASE_SLOP
    return full


def _check_unscored(dev, corp, picked, slop):
    queries = [_q(corp.queries[qi][1], corp.queries[qi][2], slop) for qi in picked]
    want = [_expect(corp, qi, slop).exists_docs for qi in picked]
    got = dev.docset(queries)
    for at, qi in enumerate(picked):
        assert np.all(got[at][:, 0] == 0)
        assert np.array_equal(got[at][:, 1], want[at]), (corp.name, corp.queries[qi][0], slop, got[at][:8, 1], want[at][:8])
    assert np.array_equal(dev.count(queries), np.array([w.size for w in want], np.uint64))
    assert int(dev.last_batch_slop_overflows(len(queries)).sum()) == 0


# ------------------------------------------------------------------------------------ 1. phrase_model's corpora
@pytest.mark.parametrize("slop", [1, 3])
@pytest.mark.parametrize("name", ["P", "T", "R", "D", "Ddel"])
def test_corpora(ta, name, slop):
    """P, T, R, D, Ddel plant position runs across 128-position blocks, vint tails, saturated tf bytes and deletes.
    Queries whose model carries a list longer than the cap (T: a first list of 254+ positions) are the overflow path:
    the batch that holds them is refused naming one of them."""
    corp = PM.corpus(name)
    every = list(range(len(corp.queries)))
    fits = [qi for qi in every if _expect(corp, qi, slop).longest <= CAP]
    over = [qi for qi in every if qi not in fits]
    # (T: its rarest term has 254+ positions in the planted docs, so every longer query there is the overflow path)
    assert {len(corp.queries[qi][1]) for qi in fits} >= ({2} if name == "T" else {2, 3, 4, 5, 8})
    assert all(len(corp.queries[qi][1]) > 2 for qi in over)
    dev = _open(ta, corp, [("docset_trees", 1)])
    try:
        _check_scored(ta, dev, corp, fits, slop)
        _check_unscored(dev, corp, fits, slop)
        if over:
            with pytest.raises(ta.TantivyAmdError) as ei:
                dev.search([_q(corp.queries[qi][1], corp.queries[qi][2], slop) for qi in fits[:2] + over], 10)
            assert "carried position list over TQ_SLOP_CARRY_CAP" in str(ei.value)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------ 2. the planted corpus S
S_MAX_DOC = TILE_DOCS + 1500 + 13
S_DFS = [150, 300, 300, 420, 500, 600, 700, 3000]
S_EDGE_DOCS = [64, 95, TILE_DOCS - 1, TILE_DOCS, S_MAX_DOC - 2]  # bit 0, bit 31, both sides of the tile boundary, the last partial word
S_BIG_DOC, S_AXBXC_DOC = 9000, 9100
S_QUERIES = [  # (name, term ids, offsets)
    ("s2", [0, 1], [0, 1]), ("s3", [0, 1, 2], [0, 1, 2]), ("gap", [0, 1, 3], [0, 1, 3]), ("last_rarest", [3, 2, 0], [0, 1, 2]),
    ("tie2", [2, 1], [0, 1]), ("tie3", [2, 1, 4], [0, 1, 2]), ("big2", [0, 4], [0, 1]), ("big3", [0, 4, 5], [0, 1, 2]),
    ("dense2", [0, 7], [0, 1]), ("dense3", [1, 7, 3], [0, 1, 2]), ("p5", [0, 1, 2, 3, 4], [0, 1, 2, 3, 4]),
    ("p8", list(range(8)), list(range(8))), ("absent", [0, PM.ABSENT, 1], [0, 1, 2]),
]


@functools.lru_cache(maxsize=None)
def build_S():
    assert S_MAX_DOC % 32 != 0
    rng = np.random.default_rng(1811)
    tp = PM._background(rng, S_MAX_DOC, S_DFS)
    for i, d in enumerate(S_EDGE_DOCS + [7000 + 97 * j for j in range(12)]):
        # every term near its place in "0 1 .. 7", the odd terms one position late (term 5: two in every other doc):
        # matches only with slop
        p = 4 + i % 7
        PM._plant(tp, d, {t: [p + t + (t % 2) + (i % 2 if t == 5 else 0)] + ([p + t + 20] if i % 3 == 0 else []) for t in range(PM.NT)})
    # a candidate doc with tf 260 in term 4 — never the first list of a query: streamed, through the saturated tf byte
    per = {t: [100 + t] for t in range(PM.NT)}
    per[4] = list(range(90, 350))
    PM._plant(tp, S_BIG_DOC, per)
    # "a x b x c": the scoring walk has no slop left for b..c at slop 1, the existence walk forgets what it spent
    PM._plant(tp, S_AXBXC_DOC, {t: [2 * t] for t in range(PM.NT)})
    filler = S_MAX_DOC - 40
    while len(tp[1]) != len(tp[2]):  # terms 1 and 2: equal doc freq, the stable tie
        t = 1 if len(tp[1]) < len(tp[2]) else 2
        while filler in tp[1] or filler in tp[2]:
            filler -= 1
        tp[t][filler] = [0]
    corp = PM.Corpus("S", tp, [40 if d % 5 else 25 for d in range(S_MAX_DOC)])
    corp.queries = S_QUERIES
    return corp


def test_planted_corpus_holds_its_edges():
    corp = build_S()
    dfs = corp.dfs()
    assert dfs[1] == dfs[2] and dfs[0] == min(dfs) and S_QUERIES[3][1][-1] == 0
    assert dfs[7] * 128 >= corp.max_doc and all(df * 128 < corp.max_doc for df in dfs[:7])  # one list with tables of its own
    assert len(corp.tp[4][S_BIG_DOC]) >= 255
    for slop in (1, 2):
        e3, e2 = _expect(corp, 1, slop), _expect(corp, 0, slop)
        for d in S_EDGE_DOCS:
            assert d in e2.docs or d in e2.exists_docs or d in e3.exists_docs
    e = _expect(corp, 1, 1)
    assert S_AXBXC_DOC in e.exists_docs and S_AXBXC_DOC not in e.docs and e.exists_docs.size > e.docs.size
    got = set()
    for qi in range(len(S_QUERIES)):
        for slop in (1, 2, 3):
            e = _expect(corp, qi, slop)
            assert e.longest <= CAP
            got |= set(int(d) for d in e.docs)
    assert got >= set(S_EDGE_DOCS) and S_BIG_DOC in got


@pytest.fixture(scope="module")
def s_dev(ta):
    corp = build_S()
    dev = _open(ta, corp, [("docset_trees", 1)])
    yield dev
    dev.close()


@pytest.mark.parametrize("slop", [1, 2, 3])
def test_planted_search_count_docset(ta, s_dev, slop):
    corp = build_S()
    every = list(range(len(S_QUERIES)))
    full = _check_scored(ta, s_dev, corp, every, slop)
    assert s_dev.segment_stats(0)["n_dense_lists"] == 1  # (every other list came through the probe pool)
    _check_unscored(s_dev, corp, every, slop)
    # k = 1, k = 10: the cut of the full rows (score desc, doc asc), pruned or not
    queries = [_q(t, o, slop) for _, t, o in S_QUERIES]
    for ex in (1, 0):
        s_dev.set_option("exhaustive", ex)
        for k in (1, 10):
            got = _rows(s_dev.search(queries, k), len(queries))
            for (gs, gd), (fs, fd) in zip(got, full):
                assert np.array_equal(gd, fd[:k]) and np.array_equal(gs, fs[:k])
        assert np.array_equal(s_dev.last_batch_match_counts(len(queries)), [f[1].size for f in full])
    s_dev.set_option("exhaustive", 1)
    if slop == 1:  # Count says the a x b x c doc exists, the scored rows do not hold it
        assert int(s_dev.count([queries[1]])[0]) > full[1][1].size


def test_planted_device_rows_and_search_one(ta, s_dev):
    import torch

    corp = build_S()
    B = ta.binding
    queries = [_q(t, o, 2) for _, t, o in S_QUERIES]
    n, k = len(queries), 16
    s_dev.prepare(queries)
    cuda = torch.device("cuda", 0)
    out = [torch.zeros((n, k), dtype=torch.float32, device=cuda), torch.zeros((n, k), dtype=torch.int32, device=cuda),
           torch.zeros((n, k), dtype=torch.int32, device=cuda), torch.zeros(n, dtype=torch.int32, device=cuda)]
    s_dev.search_prepared_device(k, out)  # tq_search_batch_device_rows: cannot report, the overflow words say
    torch.cuda.synchronize()
    assert int(s_dev.last_batch_slop_overflows(n).sum()) == 0
    assert s_dev.last_batch_stats()["kernel_mask"] == B.KERNEL_PHRASE_SLOP
    sc, dc, ct = out[0].cpu().numpy(), out[2].cpu().numpy().view(np.uint32), out[3].cpu().numpy()
    nt = sum(corp.fieldnorms)
    for qi, (name, terms, offs) in enumerate(S_QUERIES):
        e = _expect(corp, qi, 2)
        ws, wd = e.top_k(k)
        assert int(ct[qi]) == wd.size and np.array_equal(dc[qi, : wd.size], wd), name
        assert np.all(np.abs(sc[qi, : wd.size] - ws) <= 1e-5 * np.abs(ws)), name
        if PM.ABSENT in terms:
            continue
        w, cache = B.bm25_for_terms([corp.dfs()[t] for t in terms], corp.max_doc, nt)
        s1, d1, c1 = s_dev.raw_search_one(_q(terms, offs, 2), [w], cache, k)  # tq_submit + tq_wait
        assert c1 == wd.size and np.array_equal(d1[:c1], wd) and np.all(np.abs(s1[:c1] - ws) <= 1e-5 * np.abs(ws)), name


def test_mixed_batch_leaves_the_other_queries_alone(ta, s_dev):
    corp = build_S()
    plain = [(O.MODE_PHRASE, [0, 1], [0, 1]), (O.MODE_AND, [5, 6]), (O.MODE_PHRASE, [1, 7, 3], [0, 1, 2]), (O.MODE_AND, [0, 7]),
             (O.MODE_PHRASE, [0, 1], [0, 1], 0)]
    sloppy = [_q([0, 1], [0, 1], 1), _q([0, 1, 2], [0, 1, 2], 2)]
    mixed = [plain[0], sloppy[0], plain[1], plain[2], sloppy[1], plain[3], plain[4]]
    at = [0, 2, 3, 5, 6]
    want = s_dev.search(plain, 10)
    want_k = s_dev.last_batch_query_kernels(len(plain)).copy()
    got = s_dev.search(mixed, 10)
    got_k = s_dev.last_batch_query_kernels(len(mixed))
    for a, b in zip(want, got):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b[at]).view(np.uint32))
    assert np.array_equal(want_k, got_k[at]) and ta.binding.KERNEL_PHRASE_SLOP not in set(int(x) for x in want_k)
    assert int(got_k[1]) == int(got_k[4]) == ta.binding.KERNEL_PHRASE_SLOP
    rows = _rows(got, len(mixed))
    for i, (terms, slop) in ((1, ([0, 1], 1)), (4, ([0, 1, 2], 2))):
        e = SM.SlopExpect(corp.tp, terms, list(range(len(terms))), slop, corp.fieldnorms)
        ws, wd = e.top_k(10)
        assert np.array_equal(rows[i][1], wd)


# ------------------------------------------------------------------------------------ 3. random sweep
N_SWEEP = 24


@functools.lru_cache(maxsize=None)
def _sweep_case(i):
    rng = np.random.default_rng(2000 + i)
    max_doc = 1900 + int(rng.integers(0, 200))
    n_terms = int(rng.integers(6, 9))
    tp = []
    for _ in range(n_terms):
        df = int(rng.integers(40, 700))
        docs = rng.choice(max_doc, size=df, replace=False)
        tp.append({int(d): sorted(int(p) for p in rng.choice(40, size=int(rng.integers(1, 7)), replace=False)) for d in docs})
    corp = PM.Corpus("sweep%d" % i, tp, [int(x) for x in rng.integers(20, 40, size=max_doc)])
    queries = []
    for _ in range(12):
        n = int(rng.integers(2, 6))
        terms = [int(t) for t in rng.choice(n_terms, size=n, replace=False)]
        queries.append((terms, list(range(n)), int(rng.integers(0, 5))))
    return corp, queries


def _sweep_expect(corp, terms, offs, slop):
    if slop == 0:
        docs, scores, _ = PM.phrase_scores(corp.tp, terms, offs, corp.fieldnorms)
        return docs, scores, docs, 0
    e = SM.SlopExpect(corp.tp, terms, offs, slop, corp.fieldnorms)
    return e.docs, e.scores, e.exists_docs, e.longest


def test_random_sweep(ta):
    # on the CPU, before the device is asked: no case of the sweep carries a list longer than the cap
    longest = 0
    for i in range(N_SWEEP):
        corp, queries = _sweep_case(i)
        for terms, offs, slop in queries:
            longest = max(longest, _sweep_expect(corp, terms, offs, slop)[3])
    assert 0 < longest <= CAP, longest
    n_hits = n_diff = 0
    for i in range(N_SWEEP):
        corp, queries = _sweep_case(i)
        dev = _open(ta, corp, [("docset_trees", 1)])
        try:
            tuples = [_q(t, o, s) for t, o, s in queries]
            full = _rows(dev.search(tuples, K_ALL), len(tuples))
            assert int(dev.last_batch_slop_overflows(len(tuples)).sum()) == 0
            sets = dev.docset(tuples)
            assert int(dev.last_batch_slop_overflows(len(tuples)).sum()) == 0
            counts = dev.count(tuples)
            for qi, (terms, offs, slop) in enumerate(queries):
                wd, ws, we, _ = _sweep_expect(corp, terms, offs, slop)
                _assert_model(corp, "%s~%d" % (terms, slop), full[qi][0], full[qi][1], wd, ws)
                assert np.array_equal(sets[qi][:, 1], we) and int(counts[qi]) == we.size, (i, terms, slop)
                n_hits += wd.size
                n_diff += wd.size != we.size
        finally:
            dev.close()
    assert n_hits > 1000 and n_diff > 0  # (the sweep is not empty, and holds docs the two verdicts disagree on)


# ------------------------------------------------------------------------------------ 4. overflow, refusals, absent
@functools.lru_cache(maxsize=None)
def build_V():
    """Corpus R's background with one planted doc whose carried list outgrows the cap for "0 1 2" at slop 60: term 0
    once, term 1 on 45 consecutive positions (every one of them within the slop of term 0's), term 2 once."""
    base = PM.corpus("R")
    tp = [dict(t) for t in base.tp]
    PM._plant(tp, 5900, {0: [10], 1: list(range(10, 55)), 2: [14], 3: [15]})
    corp = PM.Corpus("V", tp, list(base.fieldnorms))
    return corp


V_SLOP = 60


def test_overflow_is_reported_never_a_wrong_row(ta):
    corp = build_V()
    B = ta.binding
    three, two, other = ([0, 1, 2], [0, 1, 2]), ([0, 1], [0, 1]), ([0, 1, 2], [0, 1, 2])
    e3 = SM.SlopExpect(corp.tp, *three, V_SLOP, corp.fieldnorms)
    e2 = SM.SlopExpect(corp.tp, *two, V_SLOP, corp.fieldnorms)
    eo = SM.SlopExpect(corp.tp, *other, 1, corp.fieldnorms)
    assert e3.longest > CAP and e3.longest_doc == 5900 and e2.longest == 0 and eo.longest <= CAP
    nt = sum(corp.fieldnorms)
    w3, cache = B.bm25_for_terms([corp.dfs()[t] for t in three[0]], corp.max_doc, nt)
    w2, _ = B.bm25_for_terms([corp.dfs()[t] for t in two[0]], corp.max_doc, nt)
    queries = [_q(*other, 1), _q(*three, V_SLOP), _q(*two, V_SLOP)]
    weights = [[w3], [w3], [w2]]
    dev = _open(ta, corp, [("docset_trees", 1)])
    try:
        rc, sc, dc, ct = dev.raw_search_trees(queries, weights, cache, K_ALL, opts=(1, 0), return_rc=True)
        assert rc == ERR_UNSUPPORTED and "query 1:" in _err(ta) and "carried position list over TQ_SLOP_CARRY_CAP" in _err(ta)
        over = dev.last_batch_slop_overflows(3)
        assert int(over[0]) == 0 and int(over[1]) > 0 and int(over[2]) == 0
        for qi, e in ((0, eo), (2, e2)):  # the other queries' rows are written and equal the model
            c = int(ct[qi])
            _assert_model(corp, "mate %d" % qi, sc[qi, :c], dc[qi, :c], e.docs, e.scores)
        with pytest.raises(ta.TantivyAmdError) as ei:  # tq_search_one: it fails alone ...
            dev.raw_search_one(queries[1], weights[1], cache, 10)
        assert ei.value.code == ERR_UNSUPPORTED and "TQ_SLOP_CARRY_CAP" in str(ei.value)
        s1, d1, c1 = dev.raw_search_one(queries[2], weights[2], cache, 10)  # ... and the same doc in two terms does not
        assert c1 == min(10, e2.docs.size) and np.array_equal(d1[:c1], e2.top_k(10)[1])
        # counts and doc sets report it the same way
        rc, docs, starts = dev.raw_docset(queries, 1 << 16)
        assert rc == ERR_UNSUPPORTED and "query 1:" in _err(ta) and "TQ_SLOP_CARRY_CAP" in _err(ta)
        assert np.array_equal(docs[int(starts[2]): int(starts[3])], e2.exists_docs)
        with pytest.raises(ta.TantivyAmdError):
            dev.raw_count(queries, weights, cache)
        assert np.array_equal(dev.raw_count([queries[0], queries[2]], [weights[0], weights[2]], cache), [eo.exists_docs.size, e2.exists_docs.size])
        # a MIXED count batch — the sloppy phrases go through a sub-batch of their own inside the call: the error, the
        # overflow words and the counts all stand under the caller's indices
        mixed = [(O.MODE_AND, [0, 1]), queries[2], (O.MODE_AND, [1, 2]), queries[1], queries[0]]
        qs, keep = dev._raw_scored_queries(mixed, [[1.0, 1.0], weights[2], [1.0, 1.0], weights[1], weights[0]], cache, 0)
        counts = np.full(len(mixed), 0xDEADBEEF, np.uint32)
        rc = B.lib().tq_count_batch(dev.segment_raw(0), qs, len(mixed), B._u32(counts))
        assert rc == ERR_UNSUPPORTED and "query 3:" in _err(ta) and "TQ_SLOP_CARRY_CAP" in _err(ta)
        over = dev.last_batch_slop_overflows(len(mixed))
        assert [int(x) > 0 for x in over] == [False, False, False, True, False]
        assert int(counts[1]) == e2.exists_docs.size and int(counts[4]) == eo.exists_docs.size
        assert int(counts[0]) == len(PM.and_docs(corp.tp, [0, 1])) and int(counts[2]) == len(PM.and_docs(corp.tp, [1, 2]))
        out = np.zeros(len(mixed) + 1, np.uint32)
        assert B.lib().tq_last_batch_slop_overflows(dev.segment_raw(0), B._u32(out), len(mixed) + 1) == ERR_INVALID
        qs2, keep2 = dev._raw_scored_queries(mixed[:3], [[1.0, 1.0], weights[2], [1.0, 1.0]], cache, 0)  # none over the cap
        assert B.lib().tq_count_batch(dev.segment_raw(0), qs2, 3, B._u32(counts)) == 0
        assert int(dev.last_batch_slop_overflows(3).sum()) == 0 and int(counts[1]) == e2.exists_docs.size
    finally:
        dev.close()


def test_concurrent_tickets_one_over_the_cap(ta):
    """tq_search_one from several threads at once (their queries coalesce into batches): the ticket of the overflowing
    query fails, alone, every time; its batch mates get the model's rows."""
    import ctypes as C
    import threading

    corp = build_V()
    B = ta.binding
    nt = sum(corp.fieldnorms)
    shapes = [(([0, 1, 2], [0, 1, 2]), V_SLOP), (([0, 1], [0, 1]), V_SLOP), (([0, 1, 2], [0, 1, 2]), 1), (([1, 2], [0, 1]), 2)]
    want = [SM.SlopExpect(corp.tp, *tq, slop, corp.fieldnorms) for tq, slop in shapes]
    assert want[0].longest > CAP and all(w.longest <= CAP for w in want[1:])
    k, n_threads, rounds = 10, 8, 6
    dev = _open(ta, corp, [])
    try:
        cache = B.bm25_for_terms([1], corp.max_doc, nt)[1]
        ws = [[B.bm25_for_terms([corp.dfs()[t] for t in tq[0]], corp.max_doc, nt)[0]] for tq, _ in shapes]
        # marshalled on this thread, one struct per (thread, round): the threads only make the C call
        jobs = [[i % len(shapes) if (i + r) % 3 else 0 for r in range(rounds)] for i in range(n_threads)]
        structs = [[dev._raw_scored_queries([_q(*shapes[j][0], shapes[j][1])], [ws[j]], cache, 0) for j in row] for row in jobs]
        for row in structs:
            for qs, _ in row:
                qs[0].k = k
        seg = dev.segment_raw(0)
        barrier = threading.Barrier(n_threads)
        bad = []

        def run(i):
            sc, dc, ct = np.zeros(k, np.float32), np.zeros(k, np.uint32), C.c_uint32()
            for r in range(rounds):
                barrier.wait()
                rc = B.lib().tq_search_one(seg, structs[i][r][0], None, B._f32(sc), B._u32(dc), C.byref(ct))
                j = jobs[i][r]
                if j == 0:
                    if rc != ERR_UNSUPPORTED or b"TQ_SLOP_CARRY_CAP" not in B.lib().tq_last_error():
                        bad.append((i, r, "overflow not reported", rc))
                    continue
                ws_, wd = want[j].top_k(k)
                if rc != 0 or int(ct.value) != wd.size or not np.array_equal(dc[: wd.size], wd) or \
                        not np.all(np.abs(sc[: wd.size] - ws_) <= 1e-5 * np.abs(ws_)):
                    bad.append((i, r, j, rc, int(ct.value), dc[:4].tolist(), wd[:4].tolist()))

        threads = [threading.Thread(target=run, args=(i,)) for i in range(n_threads)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not bad, bad[:5]
        assert dev.submit_stats()["queries"] >= n_threads * rounds
    finally:
        dev.close()


def test_refusals_leave_the_segment_usable(ta):
    import ctypes as C

    corp = PM.corpus("R")
    B = ta.binding
    nt = sum(corp.fieldnorms)
    w, cache = B.bm25_for_terms([corp.dfs()[0], corp.dfs()[1]], corp.max_doc, nt)
    good = _q([0, 1], [0, 1], 1)
    e = SM.SlopExpect(corp.tp, [0, 1], [0, 1], 1, corp.fieldnorms)
    dev = _open(ta, corp, [])
    try:
        def usable():
            sc, dc, ct = dev.raw_search_trees([good], [[w]], cache, K_ALL, opts=(1, 0))
            _assert_model(corp, "usable", sc[0, : int(ct[0])], dc[0, : int(ct[0])], e.docs, e.scores)

        usable()
        # a slop outside TQ_MODE_PHRASE: INVALID, by every entry point
        qs, keep = dev._raw_scored_queries([(O.MODE_AND, [0, 1])], [[1.0, 1.0]], cache, 0)
        qs[0].slop, qs[0].k = 1, 10
        out = (np.zeros(10, np.float32), np.zeros(10, np.uint32), np.zeros(1, np.uint32))
        rc = B.lib().tq_search_batch(dev.segment_raw(0), qs, 1, 10, B._f32(out[0]), B._u32(out[1]), B._u32(out[2]))
        assert rc == ERR_INVALID and "query 0" in _err(ta) and "slop" in _err(ta)
        assert B.lib().tq_count_batch(dev.segment_raw(0), qs, 1, B._u32(out[2])) == ERR_INVALID
        usable()
        # slop 256
        rc, _, _, _ = dev.raw_search_trees([_q([0, 1], [0, 1], 256)], [[w]], cache, 10, return_rc=True)
        assert rc == ERR_UNSUPPORTED and "query 0" in _err(ta) and "TQ_MAX_SLOP" in _err(ta)
        usable()
        # "docset_trees" off: refused as phrases are
        rc, _, _ = dev.raw_docset([good], 1 << 16)
        assert rc == ERR_UNSUPPORTED and "query 0" in _err(ta)
        usable()
        # scored doc sets, also under "docset_score_trees"
        for on in (0, 1):
            dev.set_option("docset_score_trees", on)
            rc, _, _, _ = dev.raw_docset_scored([good], 1 << 16, weights=[[w]], cache=cache)
            assert rc == ERR_UNSUPPORTED and "query 0" in _err(ta) and "sloppy" in _err(ta)
        usable()
        # an absent term: empty rows, count 0, TQ_OK
        absent = _q([0, PM.ABSENT], [0, 1], 2)
        sc, dc, ct = dev.raw_search_trees([absent, _q([0, PM.ABSENT, 1], [0, 1, 2], 2)], [[w], [w]], cache, 10)
        assert int(ct[0]) == int(ct[1]) == 0 and np.all(dc == 0x7FFFFFFF)
        assert np.array_equal(dev.raw_count([absent], [[w]], cache), [0])
        dev.set_option("docset_trees", 1)
        rc, _, starts = dev.raw_docset([absent, good], 1 << 16)
        assert rc == 0 and int(starts[1]) == 0 and int(starts[2]) == e.exists_docs.size
    finally:
        dev.close()


def test_other_fields_are_refused(ta):
    from tests import fields_model as FM

    fx = FM.FIXTURES["Y"]()
    dev = ta.DeviceIndex()
    try:
        dev.add_segment_fields(fx.fields)
        caches = fx.caches()
        q = _q([fx.gid(1, 0), fx.gid(1, 1)], [0, 1], 1)
        rc, _, _, _ = dev.raw_search_trees([q], [[1.0]], caches, 10, return_rc=True)
        assert rc == ERR_UNSUPPORTED and "query 0" in _err(ta) and "field" in _err(ta)
        sc, dc, ct = dev.raw_search_trees([_q([0, 1], [0, 1], 1)], [[1.0]], caches, 10)  # field 0: taken, the segment usable
        assert dev.last_batch_stats()["kernel_mask"] == ta.binding.KERNEL_PHRASE_SLOP
    finally:
        dev.close()
