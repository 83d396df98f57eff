"""GPU parity tests: the HIP path (through the C ABI / C++ host mirror) against the CPU oracle.
Doc ids and 2-term scores bit-exact; scores otherwise within 1e-5 relative (BASELINE.json)."""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import corpus_segment, random_postings, rel_close

pytestmark = pytest.mark.gpu

MODE_NAMES = {O.MODE_AND: "AND", O.MODE_OR: "OR", O.MODE_PHRASE: "PHRASE"}


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    from tests.helpers import exhaustive_by_default

    return exhaustive_by_default(tantivy_amd)


@pytest.fixture(scope="module")
def synth(ta):
    seg = O.synth_segment(200_000, n_terms=96, with_positions=True, phrase_terms=16)
    dev = ta.DeviceIndex([seg])
    yield seg, dev
    dev.close()


def _oracle_topk(seg, terms, mode, k, offsets=None):
    return O.search(seg, terms, mode, k, pruned=False, phrase_offsets=offsets)


def _device_topk(dev, queries, k):
    scores, ords, docs, counts = dev.search(queries, k)
    out = []
    for i in range(len(queries)):
        c = int(counts[i])
        out.append([(float(scores[i, j]), int(docs[i, j])) for j in range(c)])
        assert np.all(docs[i, c:] == 0x7FFFFFFF)
    return out


def _assert_hits_equal(got, want, exact=True):
    assert len(got) == len(want)
    for (gs, gd), (ws, wd) in zip(got, want):
        assert gd == wd
        if exact:
            assert np.float32(gs) == np.float32(ws), (gs, ws)
        else:
            assert rel_close(gs, ws, 1e-5)


def _assert_hits(got, want, mode, n_terms):
    """bit-exact, except unions of 3+ terms (sum order: see _assert_hits_close)"""
    if mode == O.MODE_OR and n_terms > 2:
        _assert_hits_close(got, want)
    else:
        _assert_hits_equal(got, want)


def _assert_hits_close(got, want, tol=1e-5):
    """3+ term sums: the reference's own sum order is not canonical (block_wand_union.rs sums in
    cursor order), so ranks are compared score-wise and docs up to swaps between near-ties, the
    way the reference's tests do (block_wand_union.rs:327-349).
    Which members of a tie class a row holds is checked exactly in tests/test_gpu_plateau_ties.py."""
    assert len(got) == len(want)
    for (gs, _), (ws, _) in zip(got, want):
        assert rel_close(gs, ws, tol), (gs, ws)
    wdocs = dict((d, s) for s, d in want)
    kth = want[-1][0] if want else 0.0
    for gs, gd in got:
        if gd in wdocs:
            assert rel_close(gs, wdocs[gd], tol)
        else:
            assert rel_close(gs, kth, 4 * tol), (gs, gd, kth)  # tie on the k-th score


# ------------------------------------------------------------------ codec
@pytest.mark.parametrize("use_dpp", [1, 0])
def test_decode_postings_synth(synth, use_dpp):
    seg, dev = synth
    dev.set_option("use_dpp", use_dpp)
    try:
        for t in list(range(0, 96, 5)) + [95]:
            docs, tfs = O.decode_postings(seg, t)
            gd, gt = dev.decode_postings(t, seg.terms[t].doc_freq)
            assert np.array_equal(gd, docs), "term %d docs" % t
            assert np.array_equal(gt, tfs), "term %d tfs" % t
    finally:
        dev.set_option("use_dpp", 1)


def test_decode_positions_synth(synth):
    seg, dev = synth
    for t in (0, 3, 15, 40, 95):
        docs, tfs = O.decode_postings(seg, t)
        total = int(tfs.sum())
        want, n = O.decode_positions(seg, t, total)
        assert n == total
        deltas, n2 = dev.decode_position_deltas(t, total)
        assert n2 == total
        # oracle returns per-doc prefix sums; rebuild them from the raw deltas
        ends = np.cumsum(tfs)
        starts = ends - tfs
        cs = np.cumsum(deltas.astype(np.int64))
        base = np.repeat(cs[starts] - deltas[starts].astype(np.int64), tfs)
        assert np.array_equal((cs - base).astype(np.uint32), want)


def test_decode_all_bit_widths(ta):
    """Doc-delta widths 0..31 (offset-seeded and None-seeded blocks) and tf widths 0..32,
    exact multiples of 128, vint-only lists."""
    lists = []
    for b in range(0, 31):   # block 1 starts after a gap of (1<<b)-1  => width b, offset seed
        docs = list(range(128))
        start = 127 + (1 << b)
        docs += list(range(start, start + 128)) + [start + 200, start + 300]
        tf_hi = (1 << (b + 2)) - 1 if b + 2 < 32 else 0xFFFFFFFF
        tfs = [1 + ((i * 2654435761) % tf_hi) for i in range(len(docs))]
        tfs[130] = tf_hi  # force the full tf width in block 1
        lists.append(list(zip(docs, tfs)))
    for b in range(1, 32):   # first block None-seeded with a raw first doc of b bits
        first = (1 << (b - 1)) + (12345 % (1 << (b - 1)) if b > 1 else 0)
        docs = [first + 3 * i for i in range(128)] + [first + 1000]
        lists.append([(d, 1) for d in docs])
    lists.append([(d, 0xFFFFFFFF) for d in range(0, 256, 2)])   # tf-1 needs 32 bits
    lists.append([(d, 1) for d in range(0, 128)])            # exactly one full block, doc 0 first
    lists.append([(d, 1) for d in range(5, 5 + 256)])        # two full blocks, zero-width deltas
    lists.append([(7, 3)])                                   # single posting
    lists.append([(d * 3, 1 + d % 7) for d in range(127)])   # vint only
    lists.append([(d * 2, 2) for d in range(129)])           # one block + 1 tail
    max_doc = max(pl[-1][0] for pl in lists) + 1
    seg = O.build_segment(max_doc, lists, None, record_option=O.WITH_FREQS)
    dev = ta.DeviceIndex([seg])
    try:
        for use_dpp in (1, 0):
            dev.set_option("use_dpp", use_dpp)
            for t, pl in enumerate(lists):
                gd, gt = dev.decode_postings(t, len(pl))
                assert gd.tolist() == [d for d, _ in pl], "list %d" % t
                assert gt.tolist() == [f for _, f in pl], "list %d" % t
    finally:
        dev.close()


def test_decode_basic_field_has_tf_one(ta):
    docs = sorted(set(np.random.default_rng(1).integers(0, 50_000, size=3000).tolist()))
    seg = O.build_segment(50_000, [[(d, 1) for d in docs]], None, record_option=O.BASIC)
    dev = ta.DeviceIndex([seg])
    try:
        gd, gt = dev.decode_postings(0, len(docs))
        assert gd.tolist() == docs and set(gt.tolist()) == {1}
    finally:
        dev.close()


# ------------------------------------------------------------------ AND / OR / phrase on the synthetic index
def test_and_two_terms_bit_exact(synth):
    seg, dev = synth
    rng = np.random.default_rng(5)
    pairs = [(0, 1), (1, 0), (0, 95), (94, 95), (2, 7), (10, 50), (3, 3)]
    pairs += [tuple(rng.choice(96, size=2, replace=False).tolist()) for _ in range(40)]
    got = _device_topk(dev, [(O.MODE_AND, list(p)) for p in pairs], 10)
    for p, g in zip(pairs, got):
        _assert_hits_equal(g, _oracle_topk(seg, list(p), O.MODE_AND, 10))
    # matched doc sets: stats count == oracle intersection size
    dev.search([(O.MODE_AND, [0, 1])], 10)
    st = dev.last_batch_stats()
    d, _ = O.match_all(seg, [0, 1], O.MODE_AND)
    assert st["matches"] == len(d)


def test_and_full_match_set_via_large_k(synth):
    """doc-id intersection bit-exact: ask for more hits than there are matches."""
    seg, dev = synth
    for terms in ([60, 90], [30, 95], [80, 81, 82]):
        d, s = O.match_all(seg, terms, O.MODE_AND)
        k = 1024
        assert len(d) <= k
        got = _device_topk(dev, [(O.MODE_AND, terms)], k)[0]
        assert sorted(doc for _, doc in got) == d.tolist()
        by_doc = dict((doc, sc) for sc, doc in got)
        for doc, sc in zip(d.tolist(), s.tolist()):
            assert np.float32(by_doc[doc]) == np.float32(sc)


def test_and_three_and_four_terms(synth):
    seg, dev = synth
    qs = [[0, 1, 2], [5, 1, 40], [0, 50, 95], [3, 2, 1, 0], [10, 20, 30, 40], [0, 1, 2, 3, 4]]
    got = _device_topk(dev, [(O.MODE_AND, q) for q in qs], 10)
    for q, g in zip(qs, got):
        _assert_hits_equal(g, _oracle_topk(seg, q, O.MODE_AND, 10))


@pytest.mark.parametrize("k", [1, 10, 64, 100])
def test_and_pruned_equals_exhaustive(synth, k):
    """Block-max pruning (block_wand_intersection.rs:81-85,144-165) never changes the top-k:
    same docs, same score bits, with the shared threshold (k <= 64) and without (k > 64)."""
    seg, dev = synth
    rng = np.random.default_rng(11)
    qs = [[0, 1], [1, 2], [0, 95], [2, 7, 9], [0, 1, 2, 3], [40, 41], [3, 3]]
    qs += [rng.choice(96, size=int(rng.integers(2, 5)), replace=False).tolist() for _ in range(60)]
    batch = [(O.MODE_AND, q) for q in qs]
    want = _device_topk(dev, batch, k)
    dev.set_option("exhaustive", 0)
    try:
        got = _device_topk(dev, batch, k)
        got2 = _device_topk(dev, batch, k)
    finally:
        dev.set_option("exhaustive", 1)
    dev.set_option("use_dense", 0)   # seek + decode instead of the dense-list bitmaps
    try:
        got3 = _device_topk(dev, batch, k)
        dev.set_option("exhaustive", 0)
        got4 = _device_topk(dev, batch, k)
    finally:
        dev.set_option("exhaustive", 1)
        dev.set_option("use_dense", 1)
    for q, g, g2, g3, g4, w in zip(qs, got, got2, got3, got4, want):
        assert g == w, q
        assert g2 == w, q
        assert g3 == w, q
        assert g4 == w, q
    for q, w in list(zip(qs, want))[:12]:
        _assert_hits_equal(w, _oracle_topk(seg, q, O.MODE_AND, k), exact=len(q) == 2)


@pytest.mark.parametrize("k", [1, 10, 100, 300])
def test_or_union(synth, k):
    seg, dev = synth
    rng = np.random.default_rng(k)
    qs = [[0, 1, 2, 3, 4], [90, 91, 92, 93, 94], [0, 95], [7], [95]]
    qs += [rng.choice(96, size=5, replace=False).tolist() for _ in range(8)]
    batch = [(O.MODE_OR, q) for q in qs]
    got = _device_topk(dev, batch, k)
    for q, g in zip(qs, got):
        if len(q) <= 2:
            _assert_hits_equal(g, _oracle_topk(seg, q, O.MODE_OR, k))
        else:
            _assert_hits_close(g, _oracle_topk(seg, q, O.MODE_OR, k))
    # MaxScore pruning (block_wand semantics): identical bits, with and without the bitmaps, in
    # the candidate-driven (default) and the window-parallel kernel
    for opts in ({"exhaustive": 0}, {"exhaustive": 0, "use_dense": 0}, {"use_dense": 0},
                 {"or_windows": 0}, {"or_windows": 1, "exhaustive": 0},
                 {"or_windows": 1, "exhaustive": 0, "use_dense": 0},
                 {"or_windows": 0, "use_dense": 0}):
        for name, v in opts.items():
            dev.set_option(name, v)
        try:
            got2 = _device_topk(dev, batch, k)
        finally:
            dev.set_option("exhaustive", 1)
            dev.set_option("use_dense", 1)
            dev.set_option("or_windows", -1)
        for q, g, g2 in zip(qs, got, got2):
            assert g2 == g, (q, opts)


def test_or_matches_count(synth):
    seg, dev = synth
    dev.search([(O.MODE_OR, [20, 40, 60])], 10)
    d, _ = O.match_all(seg, [20, 40, 60], O.MODE_OR)
    assert dev.last_batch_stats()["matches"] == len(d)


def test_phrase(synth):
    seg, dev = synth
    qs = [[0, 1, 2], [1, 2, 3], [5, 6, 7], [0, 1], [10, 11, 12], [2, 1, 0], [0, 5, 9], [13, 14, 15]]
    got = _device_topk(dev, [(O.MODE_PHRASE, q) for q in qs], 10)
    n_nonempty = 0
    for q, g in zip(qs, got):
        want = _oracle_topk(seg, q, O.MODE_PHRASE, 10)
        _assert_hits_equal(g, want)
        n_nonempty += bool(want)
    assert n_nonempty >= 4
    # phrase with explicit offsets ("a ? b")
    got = _device_topk(dev, [(O.MODE_PHRASE, [0, 2], [0, 2])], 10)[0]
    _assert_hits_equal(got, _oracle_topk(seg, [0, 2], O.MODE_PHRASE, 10, offsets=[0, 2]))


def test_mixed_batch_and_stride(synth):
    seg, dev = synth
    qs = [(O.MODE_AND, [0, 1]), (O.MODE_OR, [3, 4, 5]), (O.MODE_PHRASE, [0, 1, 2]),
          (O.MODE_AND, [50, 60]), (O.MODE_OR, [95]), (O.MODE_AND, [0])]
    got = _device_topk(dev, qs, 10)
    for q, g in zip(qs, got):
        _assert_hits(g, _oracle_topk(seg, q[1], q[0], 10), q[0], len(q[1]))


# ------------------------------------------------------------------ edge cases
def test_edge_cases(ta):
    rng = np.random.default_rng(9)
    md = 5000
    lists = [
        random_postings(rng, md, 100),        # 0: < 128: no skip data
        random_postings(rng, md, 128),        # 1: exactly one block
        random_postings(rng, md, 256),        # 2: two blocks, no tail
        random_postings(rng, md, 129),        # 3
        [(0, 3)],                             # 4: doc 0 only
        [(md - 1, 2)],                        # 5: last doc only
        random_postings(rng, md, 2500),       # 6
        [(d, 1) for d in range(1000, 1100)],  # 7: disjoint from 8
        [(d, 1) for d in range(3000, 3100)],  # 8
        [],                                   # 9: absent term
    ]
    fieldnorms = rng.integers(1, 400, size=md).tolist()
    seg = O.build_segment(md, lists, fieldnorms)
    dev = ta.DeviceIndex([seg])
    try:
        qs = [(O.MODE_AND, [0, 1]), (O.MODE_AND, [1, 2]), (O.MODE_AND, [2, 3]), (O.MODE_AND, [4, 6]),
              (O.MODE_AND, [5, 6]), (O.MODE_AND, [7, 8]), (O.MODE_AND, [0, 9]), (O.MODE_OR, [9]),
              (O.MODE_OR, [9, 4]), (O.MODE_OR, [4, 5]), (O.MODE_AND, [6, 6]), (O.MODE_OR, [6, 6]),
              (O.MODE_OR, [0, 1, 2, 3, 4, 5, 6, 7]), (O.MODE_AND, [6, 2, 3]), (O.MODE_AND, [4])]
        for k in (1, 3, 64, 65, 1000):
            got = _device_topk(dev, qs, k)
            for q, g in zip(qs, got):
                _assert_hits(g, _oracle_topk(seg, q[1], q[0], k), q[0], len(q[1]))
    finally:
        dev.close()


def _fuzz_segment(rng, seed, n_terms=14):
    """Random segment: dense and sparse lists, tails, runs of consecutive docs, repeated scores."""
    md = int(rng.choice([5000, 20000, 70000]))
    lists, positions = [], []
    for t in range(n_terms):
        kind = rng.integers(0, 5)
        if kind == 0:      # dense
            df = int(md * rng.uniform(0.2, 0.9))
        elif kind == 1:    # mid
            df = int(md * rng.uniform(0.01, 0.1))
        elif kind == 2:    # sparse, often below one block
            df = int(rng.integers(1, 300))
        elif kind == 3:    # exact block multiples
            df = int(128 * rng.integers(1, 6))
        else:              # a consecutive run (zero-width deltas) plus noise
            df = 0
        if df:
            docs = np.sort(rng.choice(md, size=min(df, md), replace=False))
        else:
            start = int(rng.integers(0, md // 2))
            docs = np.unique(np.concatenate([np.arange(start, start + 700),
                                             rng.choice(md, size=50, replace=False)]))
        few_tfs = rng.random() < 0.5   # few distinct tf values => many score ties
        tfs = rng.integers(1, 3 if few_tfs else 12, size=len(docs))
        lists.append(list(zip(docs.tolist(), tfs.tolist())))
        pl = []
        for tf in tfs.tolist():
            pl.append(np.sort(rng.choice(40, size=tf, replace=False)).tolist())
        positions.append(pl)
    fieldnorms = rng.integers(1, 60, size=md).tolist() if seed % 2 else [7] * md
    return O.build_segment(md, lists, fieldnorms, record_option=O.WITH_FREQS_AND_POSITIONS,
                           positions=positions)


# TQ_FUZZ_EXTRA=n: n more seeds for both fuzz tests (a soak run: `TQ_FUZZ_EXTRA=40 pytest -m gpu -k fuzz`)
_EXTRA = int(os.environ.get("TQ_FUZZ_EXTRA", "0"))


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6] + [100 + i for i in range(_EXTRA)])
def test_fuzz_random_segments(ta, seed):
    """Random segments (dense and sparse lists, tails, runs of consecutive docs, repeated scores)
    x random AND / OR / phrase queries x k, in every execution mode (pruned / exhaustive, with and
    without the dense-list bitmaps): always the oracle's exhaustive top-k."""
    rng = np.random.default_rng(1000 + seed)
    n_terms = 14
    seg = _fuzz_segment(rng, seed, n_terms)
    queries = []
    for _ in range(40):
        mode = int(rng.choice([O.MODE_AND, O.MODE_AND, O.MODE_OR, O.MODE_PHRASE]))
        n = int(rng.integers(1 if mode == O.MODE_OR else 2, 6))
        terms = rng.choice(n_terms, size=n, replace=False).tolist()
        queries.append((mode, terms))
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 16)  # terms are prepared lazily: set before the first query
        for k in (1, 10, 100):
            want = [_oracle_topk(seg, q[1], q[0], k) for q in queries]
            for ex, ud, ow in ((1, 1, 0), (0, 1, 0), (0, 0, 0), (1, 0, 0), (0, 1, 1), (1, 0, 1)):
                dev.set_option("exhaustive", ex)
                dev.set_option("use_dense", ud)
                dev.set_option("or_windows", ow)
                got = _device_topk(dev, queries, k)
                for q, g, w in zip(queries, got, want):
                    try:
                        _assert_hits(g, w, q[0], len(q[1]))
                    except AssertionError:
                        raise AssertionError("seed %d k %d exhaustive %d use_dense %d or_windows %d "
                                             "query %r\ngot  %r\nwant %r" %
                                             (seed, k, ex, ud, ow, q, g[:5], w[:5]))
        dev.set_option("or_windows", -1)
    finally:
        dev.close()


@pytest.mark.parametrize("seed", [21, 22, 23, 24] + [200 + i for i in range(_EXTRA)])
def test_fuzz_random_segments_boolean(ta, seed):
    """The same random segments under random boolean queries (occurs, nested unions,
    minimum_number_should_match), pruned / exhaustive, with and without bitmaps: the top-k and the
    match counts of the oracle's restatements (dense numpy semantics == C scorer tree)."""
    rng = np.random.default_rng(seed)
    n_terms = 14
    seg = _fuzz_segment(rng, seed, n_terms)
    queries = []
    for _ in range(48):
        n = int(rng.integers(1, 6))
        terms = rng.choice(n_terms, size=n, replace=False).tolist()
        n_cl = int(rng.integers(1, n + 1))
        cof = sorted(rng.integers(0, n_cl, size=n).tolist())
        occ_of = rng.choice([O.MUST, O.MUST, O.SHOULD, O.SHOULD, O.MUST_NOT], size=n_cl).tolist()
        occ = [int(occ_of[c]) for c in cof]
        n_should_cl = len({c for c, o in zip(cof, occ) if o == O.SHOULD})
        widest_should = max([cof.count(c) for c, o in zip(cof, occ) if o == O.SHOULD], default=1)
        msm = int(rng.integers(0, n_should_cl + 2)) if rng.random() < 0.4 else 0
        if msm >= 2 and widest_should > 1 and msm != n_should_cl:
            msm = 1  # min_should_match > 1 over nested unions stays on the CPU (Unsupported)
        queries.append((ta.MODE_BOOL, terms, occ, cof, msm))
    want_all = []
    for q in queries:
        w = _bool_want(seg, q[1], q[2], (), q[3], q[4])
        dc, _ = O.bool_match_all_c(seg, q[1], q[2], q[3], q[4])
        assert sorted(d for _, d in w) == dc.tolist(), q   # the two restatements agree
        want_all.append(w)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 16)
        for k in (1, 10, 100):
            for ex, ud in ((1, 1), (0, 1), (0, 0), (1, 0)):
                dev.set_option("exhaustive", ex)
                dev.set_option("use_dense", ud)
                got = _device_topk(dev, queries, k)
                counts = dev.last_batch_match_counts(len(queries)) if ex else None
                for i, (q, g, w) in enumerate(zip(queries, got, want_all)):
                    try:
                        _assert_hits_close(g, w[:k]) if len(w) > k else _assert_bool_hits(g, w, k, q[2], q[3])
                        if ex:
                            assert counts[i] == len(w)
                    except AssertionError:
                        raise AssertionError("seed %d k %d exhaustive %d use_dense %d query %r\ngot  %r\n"
                                             "want %r" % (seed, k, ex, ud, q, g[:5], w[:5]))
        dev.set_option("exhaustive", 1)
        dev.set_option("use_dense", 1)
    finally:
        dev.close()


def _alive_bytes(max_doc, deleted):
    """BitSet::serialize (common/src/bitset.rs:215-223) of the alive set."""
    bits = np.ones(((max_doc + 63) // 64) * 64, dtype=np.uint8)
    bits[max_doc:] = 0
    bits[np.asarray(sorted(deleted), dtype=np.int64)] = 0
    return np.uint32(max_doc).tobytes() + np.packbits(bits, bitorder="little").tobytes()


def test_deletes_and_counts(ta):
    """AliveBitSet filter (sort_by_score.rs:44-53) and per-query match counts (Count collector),
    every query shape, pruned and exhaustive."""
    seg = O.synth_segment(120_000, n_terms=48, with_positions=True, phrase_terms=12)
    rng = np.random.default_rng(77)
    deleted = set(rng.choice(seg.max_doc, size=seg.max_doc // 3, replace=False).tolist())
    queries = [(O.MODE_AND, [0, 1]), (O.MODE_AND, [2, 30]), (O.MODE_AND, [40, 41, 3]),
               (O.MODE_OR, [0, 5, 9]), (O.MODE_OR, [44]), (O.MODE_OR, [1, 2, 3, 20, 47]),
               (O.MODE_PHRASE, [0, 1, 2]), (O.MODE_PHRASE, [4, 5])]
    dev = ta.DeviceIndex([seg])
    try:
        # counts without deletes == oracle match counts
        dev.search(queries, 10)
        counts = dev.last_batch_match_counts(len(queries))
        for (mode, terms), c in zip(queries, counts.tolist()):
            d, _ = O.match_all(seg, terms, mode)
            assert c == len(d), (mode, terms)
        dev.set_alive_bitset(_alive_bytes(seg.max_doc, deleted))
        for k in (5, 100):
            want = []
            for mode, terms in queries:
                d, s = O.match_all(seg, terms, mode)
                hits = [(float(sc), int(doc)) for doc, sc in zip(d.tolist(), s.tolist())
                        if doc not in deleted]
                hits.sort(key=lambda h: (-h[0], h[1]))
                want.append(hits)
            for ex in (1, 0):
                dev.set_option("exhaustive", ex)
                got = _device_topk(dev, queries, k)
                if ex:
                    counts = dev.last_batch_match_counts(len(queries))
                for i, ((mode, terms), g, w) in enumerate(zip(queries, got, want)):
                    assert all(doc not in deleted for _, doc in g)
                    _assert_hits(g, w[:k], mode, len(terms))
                    if ex:
                        assert counts[i] == len(w), (mode, terms)
        dev.set_option("exhaustive", 1)
        # Count collector through the C ABI (tq_count_batch), deletes applied, mode untouched
        dev.set_option("exhaustive", 0)
        w1, cache = ta.bm25_for_terms([seg.terms[0].doc_freq], seg.max_doc, seg.total_num_tokens)
        cnt = dev.raw_count([(O.MODE_AND, [0, 1]), (O.MODE_OR, [0, 5, 9]), (O.MODE_PHRASE, [0, 1, 2])],
                            [[w1, w1], [w1, w1, w1], [w1]], cache)
        for (mode, terms), c in zip([queries[0], queries[3], queries[6]], cnt.tolist()):
            d, _ = O.match_all(seg, terms, mode)
            assert c == sum(1 for doc in d.tolist() if doc not in deleted), (mode, terms)
        dev.set_option("exhaustive", 1)
        # the Count collector through the host mirror (Searcher::search(&query, &Count))
        got_counts = dev.count(queries)
        for (mode, terms), c in zip(queries, got_counts.tolist()):
            d, _ = O.match_all(seg, terms, mode)
            assert c == sum(1 for doc in d.tolist() if doc not in deleted), (mode, terms)
        # clearing the bitset restores the plain results
        dev.set_alive_bitset(None)
        got = _device_topk(dev, queries[:2], 10)
        for (mode, terms), g in zip(queries[:2], got):
            _assert_hits_equal(g, _oracle_topk(seg, terms, mode, 10))
        # malformed bitsets are refused
        with pytest.raises(ta.TantivyAmdError):
            dev.set_alive_bitset(np.uint32(seg.max_doc + 1).tobytes() + bytes(8 * ((seg.max_doc + 63) // 64)))
    finally:
        dev.close()


def _bool_want(seg, terms, occurs, deleted=(), clause_of=None, msm=0):
    d, sc = O.bool_match_all(seg, terms, occurs, clause_of, msm)
    hits = [(float(x), int(doc)) for doc, x in zip(d.tolist(), sc.tolist()) if doc not in deleted]
    hits.sort(key=lambda h: (-h[0], h[1]))
    return hits


def _assert_bool_hits(got, want_all, k, occurs, clause_of=None):
    """bit-exact unless a union sums 3+ terms (union order, see O.bool_match_all)"""
    want = want_all[:k]
    n_should = sum(1 for o in occurs if o == O.SHOULD)
    widest = max(clause_of.count(c) for c in clause_of) if clause_of else 1
    # Four or more Must TERMS and nothing else: the host's weight() hands the device a TermIntersection
    # (boolean_weight.rs:330), which block_wand_intersection sums leader first, then list by list (:144-165) —
    # ((l + r) + o1) + o2 — while the scorer tree the boolean oracle restates sums Intersection::score's way
    # (intersection.rs:325-329: (l + r) + (o1 + o2)), which is what the reference's UNPRUNED collectors see
    # (boolean_weight.rs:521-528).  Both are the reference's bits, one per collector path; they differ by an ulp
    # once in a few thousand docs (fuzz seed 295, found by a 500-seed soak in round 6).
    n_must_terms = sum(1 for o in occurs if o == O.MUST)
    all_must_terms = n_must_terms == len(occurs) and widest == 1 and n_must_terms >= 4
    if all_must_terms or n_should >= 3 or widest >= 3 or (n_should == 2 and O.MUST in occurs and widest > 1):
        if len(want_all) > k:  # near-ties across the k-th rank
            _assert_hits_close(got, want)
        else:
            assert sorted(d for _, d in got) == sorted(d for _, d in want)
            _assert_hits_close(got, want)
    else:
        _assert_hits_equal(got, want)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_boolean_mixed_occurs(ta, seed):
    """Flat BooleanQuery with Must / Should / MustNot term clauses (RequiredOptionalScorer,
    Exclude; boolean_weight.rs:236-431) against the oracle's restatement: pruned and exhaustive,
    with and without bitmaps, with deletes, and the match counts."""
    rng = np.random.default_rng(seed)
    seg = O.synth_segment(60_000 + 7000 * seed, n_terms=40, with_positions=False)
    shapes = [([O.MUST, O.SHOULD]), ([O.MUST, O.MUST_NOT]), ([O.SHOULD, O.MUST_NOT]),
              ([O.MUST, O.MUST, O.SHOULD]), ([O.MUST, O.SHOULD, O.SHOULD]),
              ([O.SHOULD, O.SHOULD, O.MUST_NOT]), ([O.MUST, O.MUST, O.MUST, O.MUST_NOT]),
              ([O.MUST, O.SHOULD, O.MUST_NOT, O.SHOULD, O.MUST]),
              ([O.MUST, O.MUST, O.MUST, O.MUST, O.SHOULD]), ([O.MUST_NOT, O.SHOULD]),
              ([O.MUST_NOT, O.MUST_NOT, O.MUST]), ([O.MUST_NOT])]
    M, S, N = O.MUST, O.SHOULD, O.MUST_NOT
    # (occurs, clause_of, minimum_number_should_match): nested unions and required Should parts
    # (benches/and_or_queries.rs:150-153: `+c +(b OR d)`, `+(c OR b) +(d OR e)`)
    nested = [([M, M, M], [0, 1, 1], 0), ([M, M, M, M], [0, 0, 1, 1], 0),
              ([M, M, M, S], [0, 1, 1, 2], 0), ([M, M, M, N], [0, 0, 1, 2], 0),
              ([M, M, M, M, M], [0, 1, 1, 2, 2], 0), ([M, M, M, M], [0, 1, 1, 1], 0),
              ([M, S, S], None, 1), ([M, S, S, S], None, 2), ([S, S, S], None, 2),
              ([S, S, S], None, 3), ([S, S, N], None, 2), ([M, S], None, 1), ([M, S], None, 2),
              ([M, M], None, 1), ([S, S, S, S, N], None, 3), ([M, S, S, N], [0, 1, 1, 2], 1),
              ([N, N, S, S], [0, 0, 1, 2], 0)]
    queries = []
    for occ in shapes * 3:
        terms = rng.choice(40, size=len(occ), replace=False).tolist()
        queries.append((ta.MODE_BOOL, terms, list(occ), None, 0))
    for occ, cof, msm in nested * 2:
        terms = rng.choice(40, size=len(occ), replace=False).tolist()
        queries.append((ta.MODE_BOOL, terms, list(occ), cof, msm))
    deleted = set(rng.choice(seg.max_doc, size=seg.max_doc // 5, replace=False).tolist())
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 16)
        for dels in ((), deleted):
            dev.set_alive_bitset(_alive_bytes(seg.max_doc, dels) if dels else None)
            want = [_bool_want(seg, q[1], q[2], dels, q[3], q[4]) for q in queries]
            for k in (1, 10, 100):
                for ex, ud in ((1, 1), (0, 1), (0, 0), (1, 0)):
                    dev.set_option("exhaustive", ex)
                    dev.set_option("use_dense", ud)
                    got = _device_topk(dev, queries, k)
                    counts = dev.last_batch_match_counts(len(queries)) if ex else None
                    for i, (q, g, w) in enumerate(zip(queries, got, want)):
                        try:
                            _assert_bool_hits(g, w, k, q[2], q[3])
                            if ex:
                                assert counts[i] == len(w)
                        except AssertionError:
                            raise AssertionError("seed %d k %d exhaustive %d use_dense %d deletes %d "
                                                 "query %r\ngot  %r\nwant %r" %
                                                 (seed, k, ex, ud, bool(dels), q, g[:5], w[:5]))
        dev.set_option("exhaustive", 1)
        dev.set_option("use_dense", 1)
    finally:
        dev.close()


def test_boolean_degenerate_shapes(ta):
    """An absent Must term or MustNot clauses alone match nothing (EmptyScorer); absent Should /
    MustNot terms drop out; all-Must / all-Should boolean queries equal the AND / OR modes."""
    rng = np.random.default_rng(5)
    md = 30_000
    lists = [random_postings(rng, md, int(df)) for df in (9000, 400, 6000, 2500, 7000, 3000, 800)]
    lists.append([])  # 7: absent term
    seg = O.build_segment(md, lists, rng.integers(1, 300, size=md).tolist())
    dev = ta.DeviceIndex([seg])
    try:
        absent = 7
        qs = [(ta.MODE_BOOL, [0, absent], [O.MUST, O.MUST]),
              (ta.MODE_BOOL, [3], [O.MUST_NOT]),
              (ta.MODE_BOOL, [0, absent, 2], [O.MUST, O.SHOULD, O.MUST_NOT]),
              (ta.MODE_BOOL, [0, absent], [O.MUST, O.MUST_NOT]),
              (ta.MODE_BOOL, [4, 5, 6], [O.MUST, O.MUST, O.MUST]),
              (ta.MODE_BOOL, [4, 5], [O.SHOULD, O.SHOULD])]
        for ex in (1, 0):
            dev.set_option("exhaustive", ex)
            got = _device_topk(dev, qs, 10)
            assert got[0] == [] and got[1] == []
            _assert_hits_equal(got[2], _bool_want(seg, [0, 2], [O.MUST, O.MUST_NOT])[:10])
            _assert_hits_equal(got[3], _oracle_topk(seg, [0], O.MODE_OR, 10))
            _assert_hits_equal(got[4], _oracle_topk(seg, [4, 5, 6], O.MODE_AND, 10))
            _assert_hits_equal(got[5], _oracle_topk(seg, [4, 5], O.MODE_OR, 10))
        dev.set_option("exhaustive", 1)
    finally:
        dev.close()


def test_ties_prefer_lower_doc(ta):
    md = 1000
    lists = [[(d, 2) for d in range(0, md, 2)], [(d, 2) for d in range(0, md, 3)]]
    seg = O.build_segment(md, lists, [10] * md)  # identical scores for every match
    dev = ta.DeviceIndex([seg])
    try:
        got = _device_topk(dev, [(O.MODE_AND, [0, 1]), (O.MODE_OR, [0, 1])], 7)
        assert [d for _, d in got[0]] == [0, 6, 12, 18, 24, 30, 36]
        _assert_hits_equal(got[0], _oracle_topk(seg, [0, 1], O.MODE_AND, 7))
        _assert_hits_equal(got[1], _oracle_topk(seg, [0, 1], O.MODE_OR, 7))
    finally:
        dev.close()


def test_error_paths(synth, ta):
    seg, dev = synth
    with pytest.raises(ta.TantivyAmdError):
        dev.search([(O.MODE_PHRASE, [0])], 10)          # phrase needs >= 2 terms
    with pytest.raises(ta.TantivyAmdError):
        dev.search([(O.MODE_AND, [0, 1])], 5000)        # k above the device heap
    with pytest.raises(ta.TantivyAmdError):
        dev.search([(O.MODE_AND, list(range(20)))], 10)  # too many terms
    # the segment still works afterwards
    _assert_hits_equal(_device_topk(dev, [(O.MODE_AND, [0, 1])], 3)[0],
                       _oracle_topk(seg, [0, 1], O.MODE_AND, 3))


# ------------------------------------------------------------------ the reference's own corpora through the device
def test_reference_kat_corpora(ta):
    seg, v = corpus_segment(["Hello happy tax payer.", "Droopy says hello happy tax payer",
                             "I like Droopy"])
    dev = ta.DeviceIndex([seg])
    try:
        sc, ords, docs, cnt = dev.search([(O.MODE_OR, [v["droopy"], v["tax"]])], 4)
        assert cnt[0] == 3 and docs[0, :3].tolist() == [1, 2, 0]
        for got, want in zip(sc[0, :3], (0.81221175, 0.5376842, 0.48527452)):
            assert np.float32(got) == np.float32(want)
        sc, ords, docs, cnt = dev.search([(O.MODE_OR, [v["droopy"], v["tax"]])], 2, offset=1)
        assert docs[0, :2].tolist() == [2, 0]
    finally:
        dev.close()
    seg, v = corpus_segment(["a b c", "a b c a b"])
    dev = ta.DeviceIndex([seg])
    try:
        sc, ords, docs, cnt = dev.search([(O.MODE_PHRASE, [v["a"], v["b"]])], 10)
        assert sorted(docs[0, :2].tolist()) == [0, 1]
        by = dict(zip(docs[0, :2].tolist(), sc[0, :2].tolist()))
        assert abs(by[0] - 0.40618482) < 5e-4 and abs(by[1] - 0.46844664) < 5e-4
    finally:
        dev.close()
    seg, v = corpus_segment(["a b c", "a c", "b c", "a b c d", "d"])
    dev = ta.DeviceIndex([seg])
    try:
        sc, ords, docs, cnt = dev.search([(O.MODE_AND, [v["a"], v["b"]])], 10)
        assert docs[0, :2].tolist() == [0, 3]
        assert abs(sc[0, 0] - 0.977973) < 5e-4 and abs(sc[0, 1] - 0.84699446) < 5e-4
    finally:
        dev.close()


def test_block_wand_regression_inputs(ta):
    """The reference's pinned block-WAND inputs: the device's exhaustive top-k must agree with
    the oracle's *pruned* executors under the reference's own fuzzy comparison."""
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                       "block_wand_regressions.json")))

    def nearly(a, b):
        return abs(a - b) < 0.0001 * abs(a + b)

    for name, mode in (("union_reproduce_proptest", O.MODE_OR),
                       ("intersection_three_scorers_regression", O.MODE_AND)):
        g = gold[name]
        fn = [f for f in g["fieldnorms"] for _ in range(64)]
        pls = [[(d * 64 + o, tf if o == 0 else 1) for d, tf in pl for o in range(64)]
               for pl in g["posting_lists"]]
        seg = O.build_segment(len(fn), pls, fn)
        dev = ta.DeviceIndex([seg])
        try:
            for k in (1, 2, 3, 10):
                got = _device_topk(dev, [(mode, [0, 1, 2])], k)[0]
                want = O.search(seg, [0, 1, 2], mode, k, pruned=True)
                exact = _oracle_topk(seg, [0, 1, 2], mode, k)
                _assert_hits(got, exact, mode, 3)
                assert len(got) == len(want)
                kth = want[-1][0] if want else 0.0
                for (gs, gd), (ws, wd) in zip(got, want):
                    assert nearly(gs, ws)
                    if not nearly(ws, kth):
                        assert gd == wd
        finally:
            dev.close()


# ------------------------------------------------------------------ multi-segment merge
def test_two_segments_global_stats_and_merge(ta):
    segs = [O.synth_segment(60_000, n_terms=32, segment_ord=o) for o in range(2)]
    dev = ta.DeviceIndex(segs)
    try:
        nd = sum(s.max_doc for s in segs)
        nt = sum(s.total_num_tokens for s in segs)
        qs = [(O.MODE_AND, [0, 1]), (O.MODE_OR, [2, 9, 30]), (O.MODE_AND, [5, 20, 31])]
        sc, ords, docs, cnt = dev.search(qs, 10, offset=3)
        for qi, (mode, terms) in enumerate(qs):
            dfs = [sum(s.terms[t].doc_freq for s in segs) for t in terms]
            hits = []
            for o, s in enumerate(segs):
                w = O.default_weights(s, terms, mode, total_num_docs=nd, total_num_tokens=nt, dfs=dfs)
                for score, doc in O.search(s, terms, mode, 13, weights=w, pruned=False):
                    hits.append((score, o, doc))
            want = O.merge_top_k(hits, 3, 10)
            got = [(float(sc[qi, j]), int(ords[qi, j]), int(docs[qi, j])) for j in range(int(cnt[qi]))]
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g[1:] == w[1:]
                assert rel_close(g[0], w[0], 1e-5)
    finally:
        dev.close()


def test_pruning_is_exact_under_global_statistics(ta):
    """Block-max pairs are selected under each segment's own average fieldnorm; with the global
    statistics of a multi-segment index the device widens those bounds by (1 + d)^2
    ("bound_slack_ppm", set by the host mirror): pruned == exhaustive on every query, also when
    the segments' averages differ a lot."""
    rng = np.random.default_rng(12)
    md = 40_000
    segs = []
    for avg_len in (6, 60):  # very different average fieldnorms
        lists = [random_postings(rng, md, int(df), max_tf=6) for df in
                 (20000, 9000, 4000, 15000, 700, 12000, 2500, 30000)]
        fieldnorms = rng.integers(1, 2 * avg_len, size=md).tolist()
        segs.append(O.build_segment(md, lists, fieldnorms))
    dev = ta.DeviceIndex(segs)
    try:
        dev.set_option("dense_ratio", 16)
        qs = [(O.MODE_AND, rng.choice(8, size=2, replace=False).tolist()) for _ in range(60)]
        qs += [(O.MODE_OR, rng.choice(8, size=3, replace=False).tolist()) for _ in range(30)]
        qs += [(ta.MODE_BOOL, rng.choice(8, size=3, replace=False).tolist(), [O.MUST, O.SHOULD, O.MUST_NOT],
                None, 0) for _ in range(30)]
        for k in (1, 10):
            dev.set_option("exhaustive", 1)
            a = dev.search(qs, k)
            dev.set_option("exhaustive", 0)
            b = dev.search(qs, k)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)
        dev.set_option("exhaustive", 1)
    finally:
        dev.close()


def test_device_merge_kernel_matches_host(ta):
    import ctypes as C

    import torch

    from tantivy_amd import binding as B

    rng = np.random.default_rng(3)
    S, Q, K = 4, 37, 10
    scores = np.round(rng.random((S, Q, K)).astype(np.float32), 2)  # plenty of ties
    scores = -np.sort(-scores, axis=2)
    docs = rng.integers(0, 1000, size=(S, Q, K)).astype(np.uint32)
    counts = rng.integers(0, K + 1, size=(S, Q)).astype(np.uint32)
    for offset, limit in ((0, 10), (3, 5), (0, 64)):
        hs = np.zeros((Q, limit), np.float32)
        ho = np.zeros((Q, limit), np.uint32)
        hd = np.zeros((Q, limit), np.uint32)
        hc = np.zeros(Q, np.uint32)
        L = B.lib()
        assert L.tq_merge_topk(B._f32(scores), B._u32(docs), B._u32(counts), S, Q, K, offset, limit,
                               B._f32(hs), B._u32(ho), B._u32(hd), B._u32(hc)) == 0
        ctx = C.c_void_p()
        assert L.tq_init(None, 0, C.byref(ctx)) == 0
        ds, dd, dc = (torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
                      for a in (scores, docs, counts))
        os_ = torch.zeros((Q, limit), dtype=torch.float32, device="cuda")
        oo = torch.zeros((Q, limit), dtype=torch.int32, device="cuda")
        od = torch.zeros((Q, limit), dtype=torch.int32, device="cuda")
        oc = torch.zeros(Q, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = L.tq_merge_topk_device(ctx, 0, ds.data_ptr(), dd.data_ptr(), dc.data_ptr(), None, S, Q,
                                    K, offset, limit, os_.data_ptr(), oo.data_ptr(), od.data_ptr(),
                                    oc.data_ptr(), None)
        assert rc == 0, L.tq_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(oc.cpu().numpy().view(np.uint32), hc)
        assert np.array_equal(os_.cpu().numpy(), hs)
        assert np.array_equal(oo.cpu().numpy().view(np.uint32), ho)
        assert np.array_equal(od.cpu().numpy().view(np.uint32), hd)
        L.tq_shutdown(ctx)


# ------------------------------------------------------------------ BASELINE-size properties (10M docs)
@pytest.fixture(scope="module")
def big(ta):
    seg = O.synth_segment(10_000_000, n_terms=256)
    dev = ta.DeviceIndex([seg])
    yield seg, dev
    dev.close()


def test_full_size_and_against_oracle(big):
    seg, dev = big
    qs = [[0, 1], [0, 255], [1, 2], [100, 200], [254, 255], [3, 17]]
    got = _device_topk(dev, [(O.MODE_AND, q) for q in qs], 10)
    for q, g in zip(qs, got):
        _assert_hits_equal(g, _oracle_topk(seg, q, O.MODE_AND, 10))
    dev.search([(O.MODE_AND, [0, 1])], 10)
    st = dev.last_batch_stats()
    spec = O.QuerySpec(seg, [0, 1], O.default_weights(seg, [0, 1], O.MODE_AND), O.MODE_AND, 1)
    import ctypes as C
    n = O.lib().to_match_all(C.byref(seg.view), C.byref(spec.q), None, None, 0)
    assert st["matches"] == n


def test_full_size_properties(big):
    seg, dev = big
    qid = O.zipf_queries(400, 2, 256, seed=1234)
    sc, ords, docs, cnt = dev.search([(O.MODE_AND, q.tolist()) for q in qid], 10)
    for i in range(len(qid)):
        c = int(cnt[i])
        s, d = sc[i, :c], docs[i, :c]
        # sortedness: score desc, ties doc asc
        assert np.all(s[:-1] >= s[1:])
        tie = s[:-1] == s[1:]
        assert np.all(d[:-1][tie] < d[1:][tie])
        assert len(set(d.tolist())) == c
    # idempotence: same batch twice gives identical bytes
    sc2, _, docs2, cnt2 = dev.search([(O.MODE_AND, q.tolist()) for q in qid], 10)
    assert np.array_equal(sc, sc2) and np.array_equal(docs, docs2) and np.array_equal(cnt, cnt2)
    # k-monotonicity: top-10 is a prefix of top-50
    sc50, _, docs50, _ = dev.search([(O.MODE_AND, q.tolist()) for q in qid[:50]], 50)
    assert np.array_equal(docs50[:, :10], docs[:50]) and np.array_equal(sc50[:, :10], sc[:50])
    # a sample against the oracle
    for i in (0, 7, 99, 250):
        _assert_hits_equal([(float(sc[i, j]), int(docs[i, j])) for j in range(int(cnt[i]))],
                           _oracle_topk(seg, qid[i].tolist(), O.MODE_AND, 10))


def test_full_size_and_pruned(big):
    """10M docs: pruned == exhaustive on a Zipf query sample, and pruning really skips work."""
    seg, dev = big
    qid = O.zipf_queries(300, 2, 256, seed=4321)
    batch = [(O.MODE_AND, q.tolist()) for q in qid]
    sc, _, docs, cnt = dev.search(batch, 10)
    full = dev.last_batch_stats()["matches"]
    dev.set_option("exhaustive", 0)
    try:
        sc2, _, docs2, cnt2 = dev.search(batch, 10)
        pruned = dev.last_batch_stats()["matches"]
    finally:
        dev.set_option("exhaustive", 1)
    assert np.array_equal(cnt, cnt2) and np.array_equal(docs, docs2) and np.array_equal(sc, sc2)
    assert pruned < full // 4, (pruned, full)


@pytest.mark.parametrize("k", [65, 256, 1024])
def test_full_size_and_pruned_large_k(big, k):
    """10M docs, k above the 64 shared threshold slots (pruning then runs on each wave's own k-th
    key only, tq_api.cpp): pruned == exhaustive bits, and a sample against the oracle."""
    seg, dev = big
    qid = O.zipf_queries(60, 2, 256, seed=700 + k)
    batch = [(O.MODE_AND, q.tolist()) for q in qid] + [(O.MODE_AND, [0, 1]), (O.MODE_AND, [3, 200, 17])]
    sc, _, docs, cnt = dev.search(batch, k)
    dev.set_option("exhaustive", 0)
    try:
        sc2, _, docs2, cnt2 = dev.search(batch, k)
    finally:
        dev.set_option("exhaustive", 1)
    assert np.array_equal(cnt, cnt2) and np.array_equal(docs, docs2) and np.array_equal(sc, sc2)
    for i in (0, 31, 60):
        want = _oracle_topk(seg, batch[i][1], O.MODE_AND, k)
        _assert_hits_equal([(float(sc2[i, j]), int(docs2[i, j])) for j in range(int(cnt2[i]))], want)


def test_full_size_phrase(ta):
    """config 4 at BASELINE size: 3-word phrases on a 10M-doc segment with positions."""
    seg = O.synth_segment(10_000_000, n_terms=64, with_positions=True, phrase_terms=32)
    dev = ta.DeviceIndex([seg])
    try:
        qs = [[0, 1, 2], [5, 6, 7], [13, 14, 15], [29, 30, 31], [1, 0], [31, 2, 17]]
        got = _device_topk(dev, [(O.MODE_PHRASE, q) for q in qs], 10)
        for q, g in zip(qs, got):
            _assert_hits_equal(g, _oracle_topk(seg, q, O.MODE_PHRASE, 10))
        dev.set_option("use_dense", 0)
        got2 = _device_topk(dev, [(O.MODE_PHRASE, q) for q in qs], 10)
        assert got2 == got
    finally:
        dev.close()


def test_full_size_or_top100(big):
    seg, dev = big
    qs = [[0, 1, 2, 3, 4], [10, 50, 100, 150, 200], [251, 252, 253, 254, 255]]
    batch = [(O.MODE_OR, q) for q in qs]
    got = _device_topk(dev, batch, 100)
    for q, g in zip(qs, got):
        _assert_hits_close(g, _oracle_topk(seg, q, O.MODE_OR, 100))
    full = dev.last_batch_stats()["matches"]
    dev.set_option("exhaustive", 0)
    try:
        got2 = _device_topk(dev, batch, 100)
        pruned = dev.last_batch_stats()["matches"]
    finally:
        dev.set_option("exhaustive", 1)
    assert got2 == got
    assert pruned < full, (pruned, full)


def test_full_size_boolean(ta, big):
    """The reference's union_intersection shapes (benches/and_or_queries.rs:150-153) and a mixed
    `+a b -c` on the 10M-doc segment: against the oracle's restatement for a few queries, and
    pruned == exhaustive on a Zipf stream."""
    seg, dev = big
    M, S, N = O.MUST, O.SHOULD, O.MUST_NOT
    qs = [([40, 3, 9], [M, M, M], [0, 1, 1], 0), ([2, 30, 7, 100], [M, M, M, M], [0, 0, 1, 1], 0),
          ([5, 60, 1], [M, S, N], None, 0), ([200, 201, 0], [M, S, S], None, 1),
          ([12, 13, 14], [S, S, S], None, 2)]
    queries = [(ta.MODE_BOOL, t, o, c, m) for t, o, c, m in qs]
    for ex in (1, 0):
        dev.set_option("exhaustive", ex)
        got = _device_topk(dev, queries, 10)
        for (t, o, c, m), g in zip(qs, got):
            _assert_bool_hits(g, _bool_want(seg, t, o, (), c, m), 10, o, c)
    ids = O.zipf_queries(200, 4, 256, seed=99)
    shapes = [(3, [M, M, M], [0, 1, 1]), (4, [M, M, M, M], [0, 0, 1, 1]), (3, [M, S, N], None)]
    stream = []
    for i, q in enumerate(ids):
        nt, occ, cof = shapes[i % 3]
        stream.append((ta.MODE_BOOL, q.tolist()[:nt], occ, cof, 0))
    dev.set_option("exhaustive", 1)
    a = dev.search(stream, 10)
    dev.set_option("exhaustive", 0)
    b = dev.search(stream, 10)
    dev.set_option("exhaustive", 1)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_boosted_term_queries(synth, ta):
    """BoostQuery around term queries (boost_query.rs: the boost reaches the leaf through
    Weight::scorer(reader, boost) and Bm25Weight::boost_by), in AND / OR / boolean queries —
    negative boosts included (they switch the block-max pruning off)."""
    seg, dev = synth
    cases = [((O.MODE_AND, [0, 1]), [2.0, 0.5]), ((O.MODE_AND, [3, 20, 7]), [1.0, 3.25, 0.125]),
             ((O.MODE_OR, [2, 9]), [0.75, 4.0]), ((O.MODE_OR, [5]), [7.0]),
             ((O.MODE_AND, [4, 6]), [-1.0, 2.0])]
    for ex in (1, 0):
        dev.set_option("exhaustive", ex)
        got = _device_topk(dev, [q + ({"boosts": b},) for q, b in cases], 10)
        for (q, b), g in zip(cases, got):
            w = O.default_weights(seg, q[1], q[0], boosts=b)
            _assert_hits_equal(g, O.search(seg, q[1], q[0], 10, weights=w, pruned=False))
        M, S, N = O.MUST, O.SHOULD, O.MUST_NOT
        bq = [((ta.MODE_BOOL, [0, 5, 9], [M, S, N], None, 0), [1.5, 2.0, 1.0]),
              ((ta.MODE_BOOL, [10, 3, 4], [M, M, M], [0, 1, 1], 0), [0.5, 2.0, 3.0])]
        got = _device_topk(dev, [q + ({"boosts": b},) for q, b in bq], 10)
        for (q, b), g in zip(bq, got):
            _assert_hits_equal(g, O.bool_search(seg, q[1], q[2], 10, q[3], q[4], boosts=b))
    dev.set_option("exhaustive", 1)
