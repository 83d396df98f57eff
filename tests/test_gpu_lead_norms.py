"""GPU parity of the shared-intersection launch (tantivy_amd/csrc/tq_ashare.hip) around the leaders' norm bytes in
posting order (TermHost::lnorm_blob: byte i = fieldnorm id of posting i's doc, built by one launch the first time a
list leads queries of the shared launch) and the per-query records the launch and its merge read.

Hand-made segments of 24 000 docs (O.build_segment): leader lists whose lengths sit on both sides of the 128-doc block
and of the vint tail, eight lists with bitmaps for the other side of the intersections, fieldnorm ids that vary per
doc and include 0 and 255.  Every batch: the shared launch ran (kernel_mask), pruned == exhaustive bit for bit, doc
ids and 2-term scores equal to the oracle's exhaustive top-k bit for bit (1e-5 for 3+ terms: the sum order)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import rel_close
from tests.test_gpu_round3 import _alive_bytes, _big_tf_segment

pytestmark = pytest.mark.gpu

MD = 24_000
LEADER_DFS = [40, 128, 129, 255, 256, 257, 128 * 7 + 63]  # terms 0..6: tail only, one block, block + 1, ..., 7 blocks + tail
BIG_DFS = [12000, 10000, 9000, 8000, 6000, 5000, 4000, 3000]  # terms 7..14: bitmaps + tf bytes at dense_ratio 32
LATE_DFS = [300, 500]  # terms 15, 16: leaders that first lead in a later batch
LEADERS = list(range(len(LEADER_DFS)))
BIGS = list(range(len(LEADER_DFS), len(LEADER_DFS) + len(BIG_DFS)))
LATE = [BIGS[-1] + 1, BIGS[-1] + 2]
ALL_DFS = LEADER_DFS + BIG_DFS + LATE_DFS
SCATTERED_NORMS = 0x40000000  # "debug" work counters of tq_ashare.hip: norm bytes gathered doc by doc,
NORM_BYTES = 0x200000         # norm bytes the lanes consume


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


def _postings(rng, md, dfs):
    lists = []
    for df in dfs:
        docs = np.sort(rng.choice(md, size=df, replace=False))
        lists.append(list(zip(docs.tolist(), rng.integers(1, 5, size=df).tolist())))
    return lists


@pytest.fixture(scope="module")
def seg():
    rng = np.random.default_rng(20261017)
    lists = _postings(rng, MD, ALL_DFS)
    ids = rng.integers(1, 60, size=MD)
    ids[rng.choice(MD, size=MD // 8, replace=False)] = 0
    ids[rng.choice(MD, size=MD // 8, replace=False)] = 255
    for t in LEADERS:  # every leader holds docs of both extremes, its first and last posting among them
        docs = [d for d, _ in lists[t]]
        ids[docs[0]], ids[docs[-1]], ids[docs[len(docs) // 2]] = 255, 0, 255
    table = O.fieldnorm_table()
    # (the statistics are given: the sum of the id-255 norms would not fit the reference's u32 arithmetic)
    return O.build_segment(MD, lists, [int(table[i]) for i in ids], total_num_tokens=MD * 30, avg_fieldnorm=30.0)


class _Oracle:
    """O.match_all per distinct query, computed once per segment."""

    def __init__(self, seg):
        self.seg, self.memo = seg, {}

    def check(self, queries, got, k, deleted=None, rows=None):
        sc, docs, cnt = got
        for qi in (range(len(queries)) if rows is None else rows):
            mode, terms = queries[qi]
            key = (mode, tuple(terms))
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
def oracle(seg):
    return _Oracle(seg)


def _open(ta, seg, dense_ratio=32):
    dev = ta.DeviceIndex([seg])
    dev.set_option("ashare_min_batch", 0)  # (whatever the batch size)
    dev.set_option("dense_ratio", dense_ratio)
    return dev


def _exhaustive(dev, queries, k):
    dev.set_option("exhaustive", 1)
    ex = dev.search(queries, k)
    assert not (dev.last_batch_stats()["kernel_mask"] & 0x200)
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


def _rows(res):
    return res[0], res[2], res[3]


def _counter(dev, queries, k, bit):
    """One untimed batch with a work-counter bit of the shared launch (no counter changes a result)."""
    dev.set_option("exhaustive", 0)
    dev.set_option("debug", bit)
    try:
        dev.search(queries, k)
        return int(dev.last_batch_stats()["matches"])
    finally:
        dev.set_option("debug", -1)


def _pairs(leaders, bigs):
    qs = [(O.MODE_AND, [t, b]) for t in leaders for b in bigs]
    return qs + [(O.MODE_AND, [b, t]) for t in leaders for b in bigs[:2]]  # (the leader named second as well)


def _table_bytes(leaders):
    return sum(ALL_DFS[t] for t in leaders)


def test_leader_lengths_on_both_sides_of_a_block(ta, seg, oracle):
    """Leaders of 40 (tail only), 128, 129, 255, 256, 257 and 128 * 7 + 63 postings, ten queries each in one batch: the
    norm bytes the shared launch reads in posting order give the scores the per-doc gather gave; no norm byte of the
    batch is gathered doc by doc."""
    queries = _pairs(LEADERS, BIGS)
    dev = _open(ta, seg)
    try:
        ex = _exhaustive(dev, queries, 10)
        pr = _pruned(ta, dev, queries, 10)
        _same(pr, ex)
        oracle.check(queries, _rows(pr), 10)
        assert _counter(dev, queries, 10, SCATTERED_NORMS) == 0
        assert _counter(dev, queries, 10, NORM_BYTES) > 0
    finally:
        dev.close()


def test_a_table_is_built_once(ta, seg, oracle):
    """bitmap_bytes (the side tables' bytes) grows with the first pruned batch by at least one byte per posting of
    its leaders, not with a second identical batch, and again when new lists lead."""
    first = _pairs(LEADERS[:4], BIGS)
    third = _pairs(LATE + LEADERS[:2], BIGS)
    dev = _open(ta, seg)
    try:
        _exhaustive(dev, first + third, 10)  # (every term prepared, its bitmaps built)
        b0 = dev.segment_stats()["bitmap_bytes"]
        a = _pruned(ta, dev, first, 10)
        b1 = dev.segment_stats()["bitmap_bytes"]
        assert b1 - b0 >= _table_bytes(LEADERS[:4]), (b0, b1)
        b = _pruned(ta, dev, first, 10)
        assert dev.segment_stats()["bitmap_bytes"] == b1
        _same(a, b)
        oracle.check(first, _rows(a), 10)
        c = _pruned(ta, dev, third, 10)
        b3 = dev.segment_stats()["bitmap_bytes"]
        assert b3 - b1 >= _table_bytes(LATE), (b1, b3)
        oracle.check(third, _rows(c), 10)
        st = dev.segment_stats()
        assert st["bitmap_bytes"] + st["docmat_bytes"] + st["posdir_bytes"] <= st["dense_budget_bytes"]
    finally:
        dev.close()


def test_without_room_for_the_tables_the_norms_are_gathered(ta, seg, oracle):
    """"dense_budget_x" 0 once the bitmaps exist: no norm table fits, the batch still takes the shared launch and returns
    the rows it returns with the tables.  k = 128 over leaders of <= 257 postings and lists of <= 6 000: no query
    collects k docs, no threshold rises, every run decodes the same blocks — without tables every norm byte the lanes
    consume is gathered doc by doc, with them none is."""
    queries = _pairs(LEADERS[:6], BIGS[4:])
    got, scattered, consumed = {}, {}, {}
    for tables in (True, False):
        dev = _open(ta, seg)
        try:
            _exhaustive(dev, queries, 128)
            b0 = dev.segment_stats()["bitmap_bytes"]
            if not tables:
                dev.set_option("dense_budget_x", 0)
            got[tables] = _pruned(ta, dev, queries, 128)
            assert (dev.segment_stats()["bitmap_bytes"] > b0) == tables
            scattered[tables] = _counter(dev, queries, 128, SCATTERED_NORMS)
            consumed[tables] = _counter(dev, queries, 128, NORM_BYTES)
        finally:
            dev.close()
    _same(got[True], got[False])
    oracle.check(queries, _rows(got[False]), 128)
    assert consumed[True] == consumed[False] >= _table_bytes(LEADERS[:6])
    assert scattered[False] == consumed[False]
    assert scattered[True] == 0


def test_a_segment_without_a_fieldnorm_file_gets_no_table(ta):
    """FieldNormReader::constant: nothing to lay out in posting order; the constant id is used as before."""
    rng = np.random.default_rng(78)
    dfs = [40, 129, 257, 700, 12000, 9000, 6000, 4000]
    s = O.build_segment(MD, _postings(rng, MD, dfs), None, total_num_tokens=MD * 7, avg_fieldnorm=7.0)
    assert s.fieldnorm is None
    queries = [(O.MODE_AND, [t, b]) for t in range(4) for b in range(4, 8)]
    dev = _open(ta, s)
    try:
        ex = _exhaustive(dev, queries, 10)
        b0 = dev.segment_stats()["bitmap_bytes"]
        pr = _pruned(ta, dev, queries, 10)
        assert dev.segment_stats()["bitmap_bytes"] == b0
        _same(pr, ex)
        _Oracle(s).check(queries, _rows(pr), 10)
    finally:
        dev.close()


def test_leader_norm_tables_with_deletes(ta, seg, oracle):
    rng = np.random.default_rng(99)
    dele = np.sort(rng.choice(MD, size=MD // 3, replace=False))
    queries = _pairs(LEADERS, BIGS[:4])
    dev = _open(ta, seg)
    try:
        dev.set_alive_bitset(_alive_bytes(MD, dele.tolist()))
        ex = _exhaustive(dev, queries, 10)
        pr = _pruned(ta, dev, queries, 10)
        _same(pr, ex)
        oracle.check(queries, _rows(pr), 10, deleted=dele)
    finally:
        dev.close()


@pytest.mark.parametrize("k", [1, 10, 17, 100])
def test_query_records_of_a_mixed_batch(ta, seg, oracle, k):
    """What the launch and its merge read of a query: 2-term queries, 3- and 8-term ones (lists 2.. and their weights),
    one query 40 times (one result list, read by 40 merges), a list intersected with itself; k on both sides of the
    merge's 64-key width."""
    queries = _pairs(LEADERS, BIGS[:3])
    queries += [(O.MODE_AND, [2, 7, 9]), (O.MODE_AND, [6, 8, 14]), (O.MODE_AND, [9, 4, 12])] * 2
    queries += [(O.MODE_AND, [3] + BIGS[:7]), (O.MODE_AND, BIGS[:7] + [6])] * 2
    queries += [(O.MODE_AND, [5, 10])] * 40
    queries += [(O.MODE_AND, [8, 8]), (O.MODE_AND, [6, 6])] * 2
    dev = _open(ta, seg)
    try:
        ex = _exhaustive(dev, queries, k)
        pr = _pruned(ta, dev, queries, k)
        assert dev.last_batch_stats()["kernel_mask"] == ta.binding.KERNEL_ASHARE
        _same(pr, ex)
        oracle.check(queries, _rows(pr), k)
    finally:
        dev.close()


@pytest.mark.parametrize("k", [10, 100])
def test_saturated_tf_bytes_next_to_leader_norm_tables(ta, k):
    """tf >= 255 in the probed list: its byte says 'read the packed value', found through the query's second term."""
    s = _big_tf_segment(False)
    base = [(O.MODE_AND, [0, 1]), (O.MODE_AND, [1, 2]), (O.MODE_AND, [2, 0]), (O.MODE_AND, [3, 1]),
            (O.MODE_AND, [4, 0]), (O.MODE_AND, [4, 1, 2]), (O.MODE_AND, [3, 2, 0, 1]), (O.MODE_AND, [4, 3])]
    queries = base * 6
    dev = _open(ta, s)
    try:
        ex = _exhaustive(dev, queries, k)
        b0 = dev.segment_stats()["bitmap_bytes"]
        pr = _pruned(ta, dev, queries, k)
        assert dev.segment_stats()["bitmap_bytes"] > b0
        _same(pr, ex)
        _Oracle(s).check(queries, _rows(pr), k)
    finally:
        dev.close()


def test_two_batches_on_two_streams_share_the_tables(ta, seg, oracle):
    """tq_search_batch_device on two caller streams back to back: the second batch leads with the lists whose tables the
    first one's launches build, and is ordered behind it."""
    import torch

    qa = _pairs(LEADERS, BIGS[:4])
    qb = [(O.MODE_AND, [t, b]) for t in LEADERS for b in BIGS[4:]] * 2
    dev = _open(ta, seg)
    try:
        dev.set_option("exhaustive", 0)
        outs = []
        for qs, st in ((qa, torch.cuda.Stream()), (qb, torch.cuda.Stream())):
            d_sc = torch.empty((len(qs), 10), dtype=torch.float32, device="cuda")
            d_dc = torch.empty((len(qs), 10), dtype=torch.int32, device="cuda")
            d_ct = torch.empty(len(qs), dtype=torch.int32, device="cuda")
            dev.prepare(qs)
            dev.collect_segment_prepared_device(0, 10, d_sc, d_dc, d_ct, st.cuda_stream)
            outs.append((qs, d_sc, d_dc, d_ct))  # no synchronisation between the batches
        assert dev.last_batch_stats()["kernel_mask"] & ta.binding.KERNEL_ASHARE  # (waits for whatever is in flight)
        torch.cuda.synchronize()
        for qs, d_sc, d_dc, d_ct in outs:
            oracle.check(qs, (d_sc.cpu().numpy(), d_dc.cpu().numpy().view(np.uint32), d_ct.cpu().numpy().view(np.uint32)), 10)
    finally:
        dev.close()


def test_a_large_batch_followed_by_a_small_one(ta, seg, oracle):
    """5 000 queries, then 50: the staging blob's tables move with the batch size."""
    rng = np.random.default_rng(5)
    leaders, bigs = LEADERS + LATE, BIGS
    large = [(O.MODE_AND, [leaders[i], bigs[j]]) for i, j in zip(rng.integers(0, len(leaders), 5000), rng.integers(0, len(bigs), 5000))]
    small = [(O.MODE_AND, [bigs[j], leaders[i]]) for i, j in zip(rng.integers(0, len(leaders), 50), rng.integers(0, len(bigs), 50))]
    dev = _open(ta, seg)
    try:
        ex_large, ex_small = _exhaustive(dev, large, 10), _exhaustive(dev, small, 10)
        pr_large = _pruned(ta, dev, large, 10)
        pr_small = _pruned(ta, dev, small, 10)
        _same(pr_large, ex_large)
        _same(pr_small, ex_small)
        oracle.check(large, _rows(pr_large), 10, rows=range(0, 5000, 7))
        oracle.check(small, _rows(pr_small), 10)
    finally:
        dev.close()
