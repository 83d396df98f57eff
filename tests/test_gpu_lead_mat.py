"""GPU parity of the shared-intersection launch (tantivy_amd/csrc/tq_ashare.hip) around the leaders' doc-matrix words in
posting order (TermHost::lmat_blob: word i = docmat[doc of posting i], 1 KB per 128-doc block, filled by one launch the
first time a list under "lead_mat_cut" leads queries of the shared launch, inside "lead_mat_budget_x").

The table is a COPY of doc-matrix words, and the matrix changes whenever a term is prepared: a table is used only while
it is as fresh as the matrix (tq_segment::docmat_epoch), a stale one is refilled by the first batch that finds the matrix
unchanged since the batch before it.  Checked here: the table word for word against the matrix, rows with tables ==
rows without == exhaustive per-query run == oracle, the "gathered doc by doc" work counter, the stale batch.

Segments: 300 000 docs x 64 Zipf lists (df_r = 150 000 / (r + 1): the lists from rank 7 on are under the cut of 16), and
a hand-made one of 24 000 docs whose leaders sit on both sides of the 128-doc block and of the vint tail."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import rel_close
from tests.test_gpu_round3 import _alive_bytes

pytestmark = pytest.mark.gpu

CONSUMED_WORDS = 0x400000     # "debug" work counters of tq_ashare.hip: doc-matrix words the lanes consume,
GATHERED_WORDS = 0x20000000   # ... those among them that were gathered doc by doc out of the matrix
MD = 24_000
LEADER_DFS = [40, 128, 129, 256, 257, 128 * 7 + 63]  # terms 0..5: tail only, one block, block + 1, df % 128 == 0, ..., 7 blocks + tail
BIG_DFS = [6000, 5000, 4000, 3000]                   # terms 6..9: bitmaps + tf bytes at dense_ratio 32, above the cut of 16
LEADERS = list(range(len(LEADER_DFS)))
BIGS = list(range(len(LEADER_DFS), len(LEADER_DFS) + len(BIG_DFS)))


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


@pytest.fixture(scope="module")
def seg300k():
    return O.synth_segment(300_000, n_terms=64)


def _postings(rng, md, dfs):
    lists = []
    for df in dfs:
        docs = np.sort(rng.choice(md, size=df, replace=False))
        lists.append(list(zip(docs.tolist(), rng.integers(1, 5, size=df).tolist())))
    return lists


@pytest.fixture(scope="module")
def seg24k():
    rng = np.random.default_rng(20261020)
    ids = rng.integers(1, 60, size=MD)
    table = O.fieldnorm_table()
    return O.build_segment(MD, _postings(rng, MD, LEADER_DFS + BIG_DFS), [int(table[i]) for i in ids],
                           total_num_tokens=MD * 30, avg_fieldnorm=30.0)


class _Oracle:
    """O.match_all per distinct query, computed once per segment."""

    def __init__(self, seg):
        self.seg, self.memo = seg, {}

    def check(self, queries, got, k, deleted=None):
        sc, _, docs, cnt = got
        for qi, (mode, terms) in enumerate(queries):
            key = tuple(terms)
            if key not in self.memo:
                self.memo[key] = O.match_all(self.seg, terms, mode)
            d, s = self.memo[key]
            if deleted is not None and len(d):
                keep = ~np.isin(d, deleted)
                d, s = d[keep], s[keep]
            order = np.lexsort((d, -s.astype(np.float64)))[:k]
            want = [(float(s[i]), int(d[i])) for i in order]
            g = [(float(sc[qi, j]), int(docs[qi, j])) for j in range(int(cnt[qi]))]
            assert [x for _, x in g] == [x for _, x in want], (terms, g[:5], want[:5])
            for (gs, _), (ws, _) in zip(g, want):
                if len(terms) == 2:
                    assert np.float32(gs) == np.float32(ws), (terms, g[:5], want[:5])
                else:
                    assert rel_close(gs, ws, 1e-5)


@pytest.fixture(scope="module")
def oracle300k(seg300k):
    return _Oracle(seg300k)


def _open(ta, seg, dense_ratio=64, **opts):
    dev = ta.DeviceIndex([seg])
    dev.set_option("ashare_min_batch", 0)  # (whatever the batch size)
    dev.set_option("dense_ratio", dense_ratio)
    for name, value in opts.items():
        dev.set_option(name, value)
    return dev


def _exhaustive(ta, dev, queries, k):
    dev.set_option("exhaustive", 1)
    ex = dev.search(queries, k)
    assert not (dev.last_batch_stats()["kernel_mask"] & ta.binding.KERNEL_ASHARE)
    return ex


def _pruned(ta, dev, queries, k):
    dev.set_option("exhaustive", 0)
    pr = dev.search(queries, k)
    st = dev.last_batch_stats()
    assert st["kernel_mask"] & ta.binding.KERNEL_ASHARE, st
    return pr


def _same(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def _counter(dev, queries, k, bit):
    """One batch with a work-counter bit of the shared launch (no counter changes a result)."""
    dev.set_option("exhaustive", 0)
    dev.set_option("debug", bit)
    try:
        dev.search(queries, k)
        return int(dev.last_batch_stats()["matches"])
    finally:
        dev.set_option("debug", -1)


def _leader(seg, terms):
    """The list block_wand_intersection walks: the rarest, the first of equals."""
    return min(terms, key=lambda t: (seg.terms[t].doc_freq, terms.index(t)))


def _check_tables(dev, seg, leaders, cut=16):
    """lmat[i] == docmat[doc of posting i] for every leader under the cut, zero padding behind the last posting; the
    leaders above the cut have no table.  Returns the number of tables seen."""
    docmat = dev.term_table(0, "docmat")
    assert docmat.size == seg.max_doc
    seen = 0
    for t in sorted(set(leaders)):
        h = dev.term_handle(t)
        got = dev.term_table(h, "lmat")
        df = seg.terms[t].doc_freq
        if df * cut > seg.max_doc:
            assert got.size == 0, (t, df)
            continue
        docs, _ = O.decode_postings(seg, t)
        assert got.size == 128 * ((df + 127) // 128), (t, df, got.size)
        assert np.array_equal(got[:df], docmat[docs]), (t, df)
        assert not got[df:].any(), (t, df)
        seen += 1
    return seen


def _pairs(leaders, bigs):
    qs = [(O.MODE_AND, [t, b]) for t in leaders for b in bigs]
    return qs + [(O.MODE_AND, [b, t]) for t in leaders for b in bigs[:2]]  # (the leader named second as well)


def _stream300k(n, n_terms, seed):
    return [(O.MODE_AND, t.tolist()) for t in O.zipf_queries(n, n_terms, 64, seed=seed)]


def test_tables_hold_the_doc_matrix_words_of_their_postings(ta, seg300k):
    """After two identical batches every list that led and is under the cut has its table, word for word (every leader
    here ends in a vint tail); the denser leaders have none and keep the gather."""
    queries = _stream300k(500, 2, 21)
    dev = _open(ta, seg300k)
    try:
        a = _pruned(ta, dev, queries, 10)
        b = _pruned(ta, dev, queries, 10)
        _same(a, b)
        leaders = [_leader(seg300k, q[1]) for q in queries if q[1][0] != q[1][1]]
        assert _check_tables(dev, seg300k, leaders) >= 20
        st = dev.segment_stats()
        assert st["lead_mat_bytes"] > 0 and st["lead_mat_stale"] == 0
        assert st["derived_bytes"] == st["term_table_bytes"] + st["bitmap_bytes"] + st["docmat_bytes"] + st["posdir_bytes"] + st["lead_mat_bytes"]
    finally:
        dev.close()


def test_tables_of_leaders_around_the_block_size(ta, seg24k):
    """Leaders of 40 (tail only: one block), 128 (one block, no tail), 129, 256 (two full blocks), 257 and 959 postings:
    tables exact with zero padding, rows == exhaustive == oracle, and no word of the batch is gathered doc by doc."""
    queries = _pairs(LEADERS, BIGS)
    dev = _open(ta, seg24k, dense_ratio=32)
    try:
        ex = _exhaustive(ta, dev, queries, 10)
        pr = _pruned(ta, dev, queries, 10)
        pr2 = _pruned(ta, dev, queries, 10)
        _same(pr, ex)
        _same(pr2, ex)
        _Oracle(seg24k).check(queries, pr, 10)
        assert _check_tables(dev, seg24k, LEADERS) == len(LEADERS)
        assert _counter(dev, queries, 10, GATHERED_WORDS) == 0
        assert _counter(dev, queries, 10, CONSUMED_WORDS) > 0
    finally:
        dev.close()


def test_gathered_words_counter_with_and_without_tables(ta, seg24k):
    """k = 128 over leaders of <= 257 postings and lists of <= 6 000 of 24 000 docs: no query collects k docs, no
    threshold rises, every run consumes the same words — with the option off every one of them is gathered doc by doc,
    with tables none is; the rows are the same."""
    queries = _pairs(LEADERS[:5], BIGS)
    got, gathered, consumed = {}, {}, {}
    for budget in (4, 0):
        dev = _open(ta, seg24k, dense_ratio=32, lead_mat_budget_x=budget)
        try:
            ex = _exhaustive(ta, dev, queries, 128)
            got[budget] = _pruned(ta, dev, queries, 128)
            _same(got[budget], ex)
            assert (dev.segment_stats()["lead_mat_bytes"] > 0) == (budget > 0)
            gathered[budget] = _counter(dev, queries, 128, GATHERED_WORDS)
            consumed[budget] = _counter(dev, queries, 128, CONSUMED_WORDS)
        finally:
            dev.close()
    _same(got[4], got[0])
    assert consumed[4] == consumed[0] > 0
    assert gathered[0] == consumed[0]
    assert gathered[4] == 0


@pytest.mark.parametrize("k", [1, 10, 100])
def test_rows_with_tables_without_and_with_some(ta, seg300k, oracle300k, k):
    """2-term and 3-term queries with deletes: the pruned shared launch with tables == the exhaustive per-query run ==
    the oracle; the same rows with "lead_mat_budget_x" 0, and with a budget that holds the tables of some leaders
    only, so that tasks with and without a table run in one launch."""
    rng = np.random.default_rng(7)
    dele = np.sort(rng.choice(seg300k.max_doc, size=seg300k.max_doc // 5, replace=False))
    queries = _stream300k(300, 2, 31) + _stream300k(120, 3, 32)
    rows, mat_bytes = {}, {}
    for name, opts in (("all", {}), ("none", {"lead_mat_budget_x": 0}), ("some", {"lead_mat_budget_x": 1, "lead_mat_cut": 24})):
        dev = _open(ta, seg300k, **opts)
        try:
            dev.set_alive_bitset(_alive_bytes(seg300k.max_doc, dele.tolist()))
            if name == "all":
                rows["ex"] = _exhaustive(ta, dev, queries, k)
            _pruned(ta, dev, queries, k)  # (the tables are filled by the first batch that leads with their lists)
            rows[name] = _pruned(ta, dev, queries, k)
            mat_bytes[name] = dev.segment_stats()["lead_mat_bytes"]
            if name == "some":  # both kinds of task in the launch
                assert 0 < _counter(dev, queries, k, GATHERED_WORDS) < _counter(dev, queries, k, CONSUMED_WORDS)
            elif name == "all" and k == 10:
                leaders = [_leader(seg300k, q[1]) for q in queries if len(q[1]) == 2]  # (every 2-term query takes the shared launch)
                assert _check_tables(dev, seg300k, leaders) > 0
        finally:
            dev.close()
    assert mat_bytes["none"] == 0 < mat_bytes["some"] < mat_bytes["all"], mat_bytes
    _same(rows["all"], rows["ex"])
    _same(rows["none"], rows["ex"])
    _same(rows["some"], rows["ex"])
    oracle300k.check(queries, rows["all"], k, deleted=dele)


def test_a_stale_table_is_not_used_and_is_refilled_after_a_quiet_batch(ta, seg300k, oracle300k):
    """Tables exist; then a batch names two terms nobody has prepared — rank 5 gets a doc-matrix column, rank 40 a
    signature bit — each ANDed with an OLD leader (ranks 20 and 50).  Preparing them writes doc-matrix words of the
    leaders' docs: that batch must not read the tables (stats: stale leaders, the read-back is empty) and returns the
    oracle's rows; the next batch finds the matrix unchanged, refills them, and returns the same rows."""
    old = [(O.MODE_AND, [20, 10]), (O.MODE_AND, [50, 12]), (O.MODE_AND, [20, 14]), (O.MODE_AND, [50, 45])] * 3
    new = [(O.MODE_AND, [5, 20]), (O.MODE_AND, [40, 50]), (O.MODE_AND, [20, 5]), (O.MODE_AND, [50, 40])] * 3 + old[:4]
    dev = _open(ta, seg300k)
    try:
        _pruned(ta, dev, old, 10)
        a = _pruned(ta, dev, old, 10)
        oracle300k.check(old, a, 10)
        assert _check_tables(dev, seg300k, [20, 50]) == 2
        cols0 = dev.segment_stats()["n_docmat_columns"]
        stale = _pruned(ta, dev, new, 10)  # (prepares ranks 5 and 40 on the way)
        st = dev.segment_stats()
        assert st["n_docmat_columns"] == cols0 + 1, st
        assert st["lead_mat_stale"] == 2, st
        for t in (20, 50):
            assert dev.term_table(dev.term_handle(t), "lmat").size == 0
        oracle300k.check(new, stale, 10)
        quiet = _pruned(ta, dev, new, 10)
        assert dev.segment_stats()["lead_mat_stale"] == 0
        assert _check_tables(dev, seg300k, [20, 50]) == 2
        _same(quiet, stale)
        assert _counter(dev, new, 10, GATHERED_WORDS) == 0
    finally:
        dev.close()


def test_a_segment_without_a_fieldnorm_file_still_gets_the_tables(ta):
    """FieldNormReader::constant: no norm bytes to lay out in posting order (bitmap_bytes stays), but the doc-matrix
    words are: rows equal the exhaustive run's and the oracle's."""
    rng = np.random.default_rng(78)
    dfs = [40, 129, 257, 700, 12000, 9000, 6000, 4000]
    s = O.build_segment(MD, _postings(rng, MD, dfs), None, total_num_tokens=MD * 7, avg_fieldnorm=7.0)
    assert s.fieldnorm is None
    queries = [(O.MODE_AND, [t, b]) for t in range(4) for b in range(4, 8)]
    dev = _open(ta, s, dense_ratio=32)
    try:
        ex = _exhaustive(ta, dev, queries, 10)
        b0 = dev.segment_stats()["bitmap_bytes"]
        pr = _pruned(ta, dev, queries, 10)
        st = dev.segment_stats()
        assert st["bitmap_bytes"] == b0 and st["lead_mat_bytes"] >= 8 * sum(dfs[:4]), st
        for t in range(4):
            assert dev.term_table(dev.term_handle(t), "lnorm").size == 0
        _same(pr, ex)
        _Oracle(s).check(queries, pr, 10)
        assert _check_tables(dev, s, range(4)) == 4
        assert _counter(dev, queries, 10, GATHERED_WORDS) == 0
    finally:
        dev.close()
