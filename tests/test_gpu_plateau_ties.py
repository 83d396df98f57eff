"""Top-k ties at the cut, exact doc order on every scored path.

The plateau segments of tests/plateau_model.py give every query a handful of score classes shared by hundreds or
thousands of docs, so the k-th rank cuts a class in two and ONLY the tie-break (lower segment ordinal, then lower
doc id) decides which docs a row holds.  Thousands of docs equal to the threshold also keep every bound at or above
it: nothing is pruned, every candidate reaches the collectors, staging lists are cut in the middle of tasks, and the
result lists of every task reach the merge — on keys that differ in their doc half alone.

Every case runs pruned and exhaustive and asserts, with NO tolerance on membership or order:
  1. docs (and segment ordinals) == the model's row;      2. scores within 1e-5 of the model's float64;
  3. 2-term AND scores bit-equal to the oracle's;          4. identical score bits inside a class;
  5. pruned row == exhaustive row, bit for bit;            6. padding untouched;
  7. exhaustive match counts == the model's match sets;    8. the kernel family, per query.
The premises (class gap, straddle, class size per task) are asserted in tests/test_plateau_model_cpu.py.  The
tolerant helpers of tests/test_gpu_parity.py and tests/test_gpu_bshare.py let wrong members of a tie class pass;
this file is their strict companion."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import plateau_model as P
from tests.helpers import alive_bytes, rel_close

pytestmark = pytest.mark.gpu

TERMINATED = 0x7FFFFFFF


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


@functools.lru_cache(None)
def _rows(name, k):
    b = P.batch(name)
    return [P.row(a, k, b.copies) for a in P.answers(name)]


@functools.lru_cache(None)
def _oracle_pair_scores(name):
    """{query index: {doc: f32 score}} of the batch's 2-term intersections, from the oracle's executor."""
    b = P.batch(name)
    seg = P.CORPORA[b.corpus]().seg
    out, memo = {}, {}
    for qi, q in enumerate(b.queries):
        if q.kind != "and" or len(q.spec[0]) != 2 or b.copies != 1:
            continue
        if q not in memo:
            terms, boosts = q.spec
            w = O.default_weights(seg, list(terms), O.MODE_AND, boosts=None if boosts is None else list(boosts))
            d, s = O.match_all(seg, list(terms), O.MODE_AND, weights=w)
            memo[q] = dict(zip(d.tolist(), s))
        out[qi] = memo[q]
    return out


def _open(ta, b, **options):
    """A DeviceIndex over the batch's segment (`copies` times), options set before the first query, deletes applied.
    "dense_budget_x" 256: "dense_ratio" alone decides which lists get bitmaps and tf bytes, whatever the segment's size
    (the default budget of these small segments runs out after a few lists)."""
    seg = P.CORPORA[b.corpus]().seg
    dev = ta.DeviceIndex([seg] * b.copies)
    dev.set_option("dense_budget_x", 256)
    for name, v in options.items():
        dev.set_option(name, v)
    dev.set_option("timing", 1)
    dev.set_option("record_query_kernels", 1)
    if b.deleted:
        dev.set_alive_bitset(alive_bytes(seg.max_doc, b.deleted))
    return dev


def _search(dev, ta, b, k, exhaustive):
    """-> (rows, kernel mask, per-query kernels) of every segment's launch of one batch"""
    dev.set_option("exhaustive", exhaustive)
    res = dev.search([P.to_device(ta, q) for q in b.queries], k)
    n = len(b.queries)
    masks = [dev.last_batch_stats(o)["kernel_mask"] for o in range(b.copies)]
    kern = [dev.last_batch_query_kernels(n, o).tolist() for o in range(b.copies)]
    return res, masks, kern


def _assert_rows(b, res, k):
    """asserts 1-4 and 6 of the module docstring"""
    sc, ords, docs, cnt = res
    rows, ans = _rows(b.name, k), P.answers(b.name)
    exact = _oracle_pair_scores(b.name)
    for qi, (q, want, a) in enumerate(zip(b.queries, rows, ans)):
        c = int(cnt[qi])
        got = list(zip(ords[qi, :c].tolist(), docs[qi, :c].tolist()))
        assert got == [(o, d) for o, d, _ in want], "k %d query %d %r\ngot  %r\nwant %r" % (k, qi, q, got[:12], [(o, d) for o, d, _ in want][:12])
        assert np.all(docs[qi, c:] == TERMINATED), (k, qi, q)
        for j, (_, d, s) in enumerate(want):
            assert rel_close(float(sc[qi, j]), s, 1e-5), (k, qi, q, j, float(sc[qi, j]), s)
            if qi in exact:
                assert sc[qi, j] == exact[qi][d], (k, qi, q, d, float(sc[qi, j]), float(exact[qi][d]))
        cls = a.cls[np.searchsorted(a.docs, docs[qi, :c].astype(np.int64))]
        bits = sc[qi, :c].view(np.uint32)
        for cl in set(cls.tolist()):
            assert len(set(bits[cls == cl].tolist())) == 1, (k, qi, q, cl, sc[qi, :c][cls == cl])


def _assert_equal_bits(x, y, what):
    for a, bb in zip(x, y):
        assert np.array_equal(a.view(np.uint32), bb.view(np.uint32)), what


def _assert_counts(dev, b):
    """assert 7: the exhaustive run visited every alive match"""
    n = len(b.queries)
    want = [len(a.docs) for a in P.answers(b.name)]
    for o in range(b.copies):
        assert dev.last_batch_match_counts(n, o).tolist() == want, (b.name, o)


def _both_modes(dev, ta, b, k, want_pruned, want_exhaustive, twice=False):
    """One batch pruned (twice: thresholds start from zero again, same bits) and exhaustive; asserts 1-8.
    want_*: the kernel family of every query (an int) or per query (a list)."""
    n = len(b.queries)
    pr, masks, kern = _search(dev, ta, b, k, 0)
    for o in range(b.copies):
        want = want_pruned if isinstance(want_pruned, list) else [want_pruned] * n
        assert kern[o] == want, (b.name, k, o, [(i, b.queries[i], ta.binding.kernel_names(kk)) for i, (kk, w) in enumerate(zip(kern[o], want)) if kk != w][:8])
        assert masks[o] == functools.reduce(int.__or__, want), (b.name, k, o, masks[o])
    _assert_rows(b, pr, k)
    if twice:
        again, _, _ = _search(dev, ta, b, k, 0)
        _assert_equal_bits(pr, again, (b.name, k, "second identical batch"))
    ex, masks, kern = _search(dev, ta, b, k, 1)
    for o in range(b.copies):
        want = want_exhaustive if isinstance(want_exhaustive, list) else [want_exhaustive] * n
        assert kern[o] == want, (b.name, k, o, [(i, b.queries[i], ta.binding.kernel_names(kk)) for i, (kk, w) in enumerate(zip(kern[o], want)) if kk != w][:8])
        assert masks[o] == functools.reduce(int.__or__, want), (b.name, k, o, masks[o])
    _assert_counts(dev, b)
    _assert_rows(b, ex, k)
    _assert_equal_bits(pr, ex, (b.name, k, "pruned == exhaustive"))


def _is_dense(corpus, t, dense_ratio):
    return corpus.df(t) * dense_ratio >= corpus.max_doc  # (dense_candidate, tq_internal.hpp)


# ------------------------------------------------------------------------------------------ intersections
@pytest.fixture(scope="module")
def and_devs(ta):
    """(per-query kernels, shared launch) over the periodic segment: dense_ratio 64 gives the five periodic lists
    bitmaps and leaves the rare ones sparse"""
    b = P.batch("per_query_ands")
    per_query = _open(ta, b, dense_ratio=64, ashare_min_batch=1 << 20)
    shared = _open(ta, P.batch("shared_ands"), dense_ratio=64, ashare_min_batch=0)
    yield per_query, shared
    per_query.close()
    shared.close()


@pytest.mark.parametrize("use_dense", [1, 0])
@pytest.mark.parametrize("k", P.batch("per_query_ands").ks)
def test_per_query_intersections(ta, and_devs, k, use_dense):
    """tq_and.hip: the shared-threshold path (k <= 64) and the registers alone (k > 64), over the bitmaps
    (and_dense; a sparse non-leader list: and) and with seek + decode ("use_dense" 0: and)."""
    dev, _ = and_devs
    b = P.batch("per_query_ands")
    c = P.periodic()
    B = ta.binding
    want = []
    for q in b.queries:
        others = sorted(q.spec[0], key=c.df)[1:]  # (stable: the first of the rarest leads)
        want.append(B.KERNEL_AND_DENSE if use_dense and all(_is_dense(c, t, 64) for t in others) else B.KERNEL_AND)
    dev.set_option("use_dense", use_dense)
    try:
        _both_modes(dev, ta, b, k, want, want)
    finally:
        dev.set_option("use_dense", 1)


@pytest.mark.parametrize("k", P.batch("shared_ands").ks)
def test_shared_intersections(ta, and_devs, k):
    """tq_ashare.hip: 211 distinct 2- to 4-term intersections + 30 twins, three leaders with 51 to 76 distinct queries
    each (two and three groups of leads), every query in the shared launch; k on both sides of the 64-slot / 256-slot threshold rows (16 /
    17) and of one / two keys per lane (64 / 100)."""
    _, dev = and_devs
    B = ta.binding
    _both_modes(dev, ta, P.batch("shared_ands"), k, B.KERNEL_ASHARE, B.KERNEL_AND_DENSE, twice=True)


# ------------------------------------------------------------------------------------------ boolean leads
@pytest.fixture(scope="module")
def eq_dev(ta):
    """The equal-df segment with the boolean batch's deletes, every list with a bitmap (as test_gpu_bshare._all_dense)"""
    dev = _open(ta, P.batch("shared_bools"), dense_ratio=4096)
    yield dev
    dev.close()


@pytest.mark.parametrize("k", P.batch("shared_bools").ks)
def test_boolean_leads(ta, eq_dev, k):
    """tq_ashare.hip's boolean leads: `+a b -c`, `+a +(b OR c)`, `+(a OR b) +(c OR d)` and minimum_number_should_match
    over lists of one weight; the lowest docs of every cut class are deleted."""
    B = ta.binding
    _both_modes(eq_dev, ta, P.batch("shared_bools"), k, B.KERNEL_BSHARE, B.KERNEL_BOOL, twice=True)


# ------------------------------------------------------------------------------------------ unions
@pytest.fixture(scope="module")
def union_devs(ta):
    """dense_ratio 200 on the periodic segment: list 6 (300 docs) gets a bitmap, list 5 (129 docs) does not; the 40
    doc-matrix columns are reserved for the 40 longest lists, so neither rare list has one.  "xunion_ratio" 0: the
    exhaustive runs stay on the window kernel."""
    per = _open(ta, P.batch("shared_unions_periodic"), dense_ratio=200, xunion_ratio=0)
    eq = _open(ta, P.batch("shared_unions_equal_df"), dense_ratio=64, xunion_ratio=0)
    yield per, eq
    per.close()
    eq.close()


@pytest.mark.parametrize("k", P.batch("shared_unions_periodic").ks)
def test_shared_unions_periodic(ta, union_devs, k):
    """tq_ushare.hip: 1- to 4-term unions, boosted variants, one list without a bitmap and one with a bitmap but no
    doc-matrix column (both through their signature bits); k on both sides of the 64-slot / 256-slot rows, up to the
    largest staging list (128)."""
    dev, _ = union_devs
    B = ta.binding
    _both_modes(dev, ta, P.batch("shared_unions_periodic"), k, B.KERNEL_USHARE, B.KERNEL_OR_WINDOWS, twice=True)
    info = {t: dev.term_table_info(dev.term_handle(t))["has_freq"] for t in (0, 5, 6)}
    dense = {t: dev.term_table(dev.term_handle(t), "dense").size for t in (0, 5, 6)}
    assert (info[0] >> 8) & 0xFF and dense[0]                                     # a column and a bitmap
    assert not (info[5] >> 8) & 0xFF and (info[5] >> 16) & 0xFF and not dense[5]  # a signature bit, no bitmap
    assert not (info[6] >> 8) & 0xFF and (info[6] >> 16) & 0xFF and dense[6]      # a signature bit and a bitmap


@pytest.mark.parametrize("k", P.batch("shared_unions_equal_df").ks)
def test_shared_unions_equal_df(ta, union_devs, k):
    """tq_ushare.hip: 2- to 8-term unions of lists with ONE weight — the order of the leads is a tie too"""
    _, dev = union_devs
    B = ta.binding
    _both_modes(dev, ta, P.batch("shared_unions_equal_df"), k, B.KERNEL_USHARE, B.KERNEL_OR_WINDOWS, twice=True)


@pytest.mark.parametrize("name", ["per_query_unions", "per_query_unions_equal_df"])
def test_per_query_unions(ta, name):
    """tq_union.hip: the candidate-driven kernel above the shared launch's k (129, 300; pruned), the window kernel
    ("or_windows" 1; pruned and exhaustive), and the doc-major launch (tq_xunion.hip; exhaustive, k <= 128)."""
    b = P.batch(name)
    B = ta.binding
    dev = _open(ta, b, dense_ratio=64, xunion_ratio=0)
    try:
        for k in b.ks:
            if k > 128:
                _both_modes(dev, ta, b, k, B.KERNEL_UNION, B.KERNEL_OR_WINDOWS)
            dev.set_option("or_windows", 1)
            _both_modes(dev, ta, b, k, B.KERNEL_OR_WINDOWS, B.KERNEL_OR_WINDOWS)
            dev.set_option("or_windows", -1)
        dev.set_option("xunion_min_queries", 1)
        dev.set_option("xunion_ratio", 1 << 30)
        for k in (10, 128):
            ex, masks, kern = _search(dev, ta, b, k, 1)
            assert kern[0] == [B.KERNEL_XUNION] * len(b.queries) and masks[0] == B.KERNEL_XUNION, (k, masks, kern)
            _assert_counts(dev, b)
            _assert_rows(b, ex, k)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ nested trees, phrases
@pytest.mark.parametrize("k", P.batch("trees").ks)
def test_nested_trees(ta, k):
    """tq_tree.hip: `+a +((+b +c) d)`, `+a +(b c d)~2`, `(+a +b) (+c +d) (+e +f +g)` over lists of one weight"""
    b = P.batch("trees")
    dev = _open(ta, b, dense_ratio=4096)
    try:
        _both_modes(dev, ta, b, k, ta.binding.KERNEL_TREE, ta.binding.KERNEL_TREE, twice=True)
    finally:
        dev.close()


@pytest.mark.parametrize("config", ["sweep", "sparse"])
def test_phrases_of_one_class(ta, config):
    """Every match of the phrase has a phrase count of 1 under one fieldnorm: the whole match set is ONE class.
    All lists with bitmaps: the bitmap-AND sweep (phrase_sweep_kernel); no bitmaps: phrase_kernel."""
    b = P.batch("phrases")
    B = ta.binding
    dev = _open(ta, b, dense_ratio=64 if config == "sweep" else 1)
    try:
        assert P.answers("phrases")[0].n_classes == 1
        want = B.KERNEL_PHRASE_SWEEP if config == "sweep" else B.KERNEL_PHRASE
        for k in b.ks:
            _both_modes(dev, ta, b, k, want, want, twice=True)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------ two segments
@pytest.mark.parametrize("name,pruned,exhaustive", [("two_segment_ands", "KERNEL_ASHARE", "KERNEL_AND_DENSE"),
                                                    ("two_segment_unions", "KERNEL_USHARE", "KERNEL_OR_WINDOWS")])
def test_two_segments(ta, name, pruned, exhaustive):
    """The same plateau segment twice in one index: every class is split between the segments, and a tie goes to
    the lower segment ordinal before the lower doc (the merge of the segments' rows)."""
    b = P.batch(name)
    dev = _open(ta, b, dense_ratio=200 if "unions" in name else 64, ashare_min_batch=0, xunion_ratio=0)
    try:
        for k in b.ks:
            _both_modes(dev, ta, b, k, getattr(ta.binding, pruned), getattr(ta.binding, exhaustive), twice=True)
    finally:
        dev.close()
