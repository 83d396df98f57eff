"""Term preparation through the raw C ABI: tq_term_prepare_batch (its stages: known terms, the walk off the lock with
helper threads, dense lists one by one, one staged upload, directories and signature bits, terms named twice), against
tq_term_prepare with the host walk and with the device walk.

One crafted segment holds every kind of list the paths distinguish (max_doc 65 536, dense_ratio 128, TQ_RDIR_MIN_DF 256):
lists without a side table (1 .. 255 postings), lists that get a range directory (256 .. 511), dense lists (512, 2 000),
and 600 lists of 1-5 postings — one call naming 512 or more new non-dense lists is the smallest that starts a second
walker thread."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

MAX_DOC = 65_536
PLAIN, RDIR, DENSE = [1, 40, 127, 128, 129, 255], [256, 300, 511], [512, 2000]
SHAPED = PLAIN + RDIR + DENSE
N_SMALL = 600
K = 10
TQ_ERR_INVALID, TQ_ERR_FORMAT = 1, 3


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


def build_world():
    rng = np.random.default_rng(4242)
    # (every list draws its docs from one pool of 2 500, the last doc of the segment among them: two random lists of a
    # few dozen postings out of 65 536 docs would intersect in nothing)
    pool = np.sort(np.append(rng.choice(MAX_DOC - 1, size=2499, replace=False), MAX_DOC - 1))

    def draw(df):
        docs = np.sort(rng.choice(pool, size=df, replace=False))
        return list(zip(docs.tolist(), rng.integers(1, 7, size=df).tolist()))

    lists = [draw(df) for df in SHAPED] + [draw(int(rng.integers(1, 6))) for _ in range(N_SMALL)]
    seg = O.build_segment(MAX_DOC, lists, fieldnorms=rng.integers(1, 60, size=MAX_DOC).tolist())
    queries = [(O.MODE_AND, [a, b]) for a, b in itertools.permutations(range(len(SHAPED)), 2)]
    n_and = len(queries)
    queries += [(O.MODE_OR, rng.permutation(len(lists))[:3].tolist()) for _ in range(40)]
    want = [O.search(seg, q[1], q[0], K, pruned=False) for q in queries]
    return seg, lists, queries, n_and, want


@pytest.fixture(scope="module")
def world():
    """(segment, lists, queries, number of 2-term ANDs among them, oracle rows): built once, shared by the tests, never changed."""
    return build_world()


def _infos(ta, seg, ids):
    arr = (ta.binding.TqTermInfo * max(1, len(ids)))()
    for i, t in enumerate(ids):
        ti = seg.terms[t]
        arr[i].postings_off, arr[i].postings_len = ti.postings_start, ti.postings_end - ti.postings_start
        arr[i].positions_off, arr[i].positions_len = ti.positions_start, ti.positions_end - ti.positions_start
        arr[i].doc_freq = ti.doc_freq
    return arr


def _prepare_batch(ta, dev, infos, n):
    out = np.full(max(1, n), 0xFFFFFFFF, np.uint32)
    rc = ta.binding.lib().tq_term_prepare_batch(dev.segment_raw(), infos, n, ta.binding._u32(out))
    return rc, out[:n].tolist()


def _prepare_one(ta, dev, seg, t):
    ti = seg.terms[t]
    h = C.c_uint32(0xFFFFFFFF)
    rc = ta.binding.lib().tq_term_prepare(dev.segment_raw(), ti.postings_start, ti.postings_end - ti.postings_start,
                                          ti.positions_start, ti.positions_end - ti.positions_start, ti.doc_freq, C.byref(h))
    assert rc == 0, ta.binding.lib().tq_last_error()
    return int(h.value)


def _rows(out, qi):
    sc, _, dc, ct = out
    return [(float(sc[qi, j]), int(dc[qi, j])) for j in range(int(ct[qi]))]


def _check_against_oracle(queries, n_and, want, got):
    for qi, q in enumerate(queries):
        rows = _rows(got, qi)
        if qi < n_and:  # two lists: one summation order, bit-exact
            assert rows == [(float(np.float32(s)), d) for s, d in want[qi]], (q, rows[:3], want[qi][:3])
        else:  # three lists: the reference sums in cursor order (1e-5 relative, BASELINE.json); near-ties may swap
            assert sorted(d for _, d in rows) == sorted(d for _, d in want[qi]), (q, rows, want[qi])
            for (a, _), (b, _) in zip(rows, want[qi]):
                assert abs(a - b) <= 1e-5 * max(abs(a), abs(b)), (q, rows, want[qi])


def test_one_call_mixing_every_kind_of_list(ta, world):
    seg, lists, _, _, _ = world
    dev = ta.DeviceIndex([seg])
    try:
        pre, dense_twice, sparse_twice = SHAPED.index(300), SHAPED.index(2000), SHAPED.index(40)
        h_pre = _prepare_one(ta, dev, seg, pre)
        ids = list(range(len(lists))) + [dense_twice, sparse_twice]
        infos = _infos(ta, seg, ids)
        rc, out = _prepare_batch(ta, dev, infos, len(ids))
        assert rc == 0, ta.binding.lib().tq_last_error()
        by_term = {}
        for t, h in zip(ids, out):
            assert h != 0xFFFFFFFF
            assert by_term.setdefault(t, h) == h, (t, h, by_term[t])  # equal postings_off: equal handle
        assert len(set(by_term.values())) == len(lists)
        assert by_term[pre] == h_pre
        # handles in the order of the call's side effects: its dense lists first, in order, then its walked lists in order
        dense = [t for t in range(len(lists)) if len(lists[t]) >= MAX_DOC // 128]
        walked = [t for t in range(len(lists)) if t != pre and t not in dense]
        assert [by_term[t] for t in dense + walked] == list(range(h_pre + 1, h_pre + len(lists)))
        stats = dev.segment_stats(0)
        assert stats["n_dense_lists"] == len(DENSE) and stats["n_terms"] == len(lists)
        rc, again = _prepare_batch(ta, dev, infos, len(ids))
        assert rc == 0 and again == out
        assert dev.segment_stats(0)["term_table_bytes"] == stats["term_table_bytes"]
        assert [_prepare_one(ta, dev, seg, t) for t in ids] == out
    finally:
        dev.close()


def test_batch_host_walk_and_device_walk_prepare_alike(ta, world):
    seg, lists, queries, n_and, want = world
    ref = None
    for path in ("batch", "one by one", "device walk"):
        dev = ta.DeviceIndex([seg])
        try:
            dev.set_option("ashare_min_batch", 1)
            ids = list(range(len(lists)))
            if path == "batch":
                rc, out = _prepare_batch(ta, dev, _infos(ta, seg, ids), len(ids))
                assert rc == 0, ta.binding.lib().tq_last_error()
            else:
                dev.set_option("device_prepare", 1 if path == "device walk" else 0)
                out = [_prepare_one(ta, dev, seg, t) for t in ids]
            assert sorted(out) == list(range(len(lists))), path
            for t in range(len(SHAPED)):
                docs, tfs = dev.decode_postings(t, len(lists[t]))
                assert list(zip(docs.tolist(), tfs.tolist())) == lists[t], (path, t)
            dev.set_option("exhaustive", 0)
            pr = dev.search(queries, K)
            dev.set_option("exhaustive", 1)
            ex = dev.search(queries, K)
        finally:
            dev.close()
        assert np.array_equal(pr[2][:n_and], ex[2][:n_and]) and np.array_equal(pr[0][:n_and], ex[0][:n_and]), path
        assert np.array_equal(pr[3], ex[3]) and np.array_equal(pr[2], ex[2]), path
        assert np.allclose(pr[0], ex[0], rtol=1e-5, atol=0), path
        if ref is None:
            ref = pr
            _check_against_oracle(queries, n_and, want, pr)
        else:
            for a, b in zip(pr, ref):
                assert np.array_equal(a, b), path


def test_a_failed_call_leaves_the_segment_usable(ta, world):
    """Nothing is asserted about which handles a failed call left registered (ADVICE: an open finding)."""
    seg, lists, queries, n_and, want = world
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("ashare_min_batch", 1)
        ids = list(range(len(SHAPED), len(SHAPED) + 40))
        infos = _infos(ta, seg, ids)
        infos[20].doc_freq = 0
        rc, _ = _prepare_batch(ta, dev, infos, len(ids))
        assert rc == TQ_ERR_INVALID, (rc, ta.binding.lib().tq_last_error())
        ids = list(range(len(SHAPED) + 40, len(SHAPED) + 80))
        infos = _infos(ta, seg, ids)
        infos[20].postings_off = seg.idx_len - 8 - 2  # [off, off + len) ends past the idx body
        infos[20].postings_len = 16
        rc, _ = _prepare_batch(ta, dev, infos, len(ids))
        assert rc == TQ_ERR_FORMAT, (rc, ta.binding.lib().tq_last_error())
        assert b"outside the idx body" in ta.binding.lib().tq_last_error()
        ids = list(range(len(lists)))
        rc, out = _prepare_batch(ta, dev, _infos(ta, seg, ids), len(ids))
        assert rc == 0, ta.binding.lib().tq_last_error()
        assert len(set(out)) == len(lists) and 0xFFFFFFFF not in out
        dev.set_option("exhaustive", 1)
        _check_against_oracle(queries, n_and, want, dev.search(queries, K))
    finally:
        dev.close()
