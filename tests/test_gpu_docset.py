"""GPU parity of full doc sets (tantivy_amd/csrc/tq_docset.hip; Weight::for_each_no_score -> collect_block with the
alive filter: src/query/weight.rs:23-35,101-121, src/collector/mod.rs:186-221, docset_collector.rs:26-57): every
alive matching doc of a query, ascending, as CSR rows — exactly the oracle's doc sets.  Covers the tile / word /
segment-tail boundaries, every flat boolean shape including "at least m of n", lists with and without a bitmap, the
capacity protocol, sub-batching, the refusals, the device-output variant and the multi-segment host mirror."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gpu_bshare import SHAPES
from tests.test_gpu_round3 import _alive_bytes

pytestmark = pytest.mark.gpu

M, S, N = O.MUST, O.SHOULD, O.MUST_NOT
ERR_INVALID, ERR_UNSUPPORTED = 1, 4
GUARD = 0xDEADBEEF


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


@functools.lru_cache(maxsize=None)
def _synth(max_doc, n_terms, segment_ord=0, with_positions=False):
    return O.synth_segment(max_doc, n_terms=n_terms, segment_ord=segment_ord, with_positions=with_positions)


def _want(seg, q, deleted=()):
    """The oracle's ascending doc set of one query, deleted docs removed."""
    if q[0] == O.MODE_BOOL:
        d, _ = O.bool_match_all(seg, q[1], q[2], q[3] if len(q) > 3 else None, q[4] if len(q) > 4 else 0)
    else:
        d, _ = O.match_all(seg, q[1], q[0])
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


def _all_dense(dev):
    dev.set_option("dense_ratio", 4096)    # every list gets a bitmap ...
    dev.set_option("dense_budget_x", 256)  # ... whatever the segment's size


def _random_queries(ta, rng, n_terms):
    queries = []
    for occ, cof, msm in SHAPES + [([S] * 4, None, 2), ([S] * 4 + [M], None, 3), ([S, S, S], [0, 0, 1], 2)]:
        terms = rng.choice(n_terms, size=len(occ), replace=False).tolist()
        queries.append((ta.MODE_BOOL, terms, list(occ), cof, msm))
    for n in (1, 2, 3, 5):
        for _ in range(6):
            terms = rng.choice(n_terms, size=n, replace=False).tolist()
            queries.append((O.MODE_AND, terms))
            queries.append((O.MODE_OR, terms))
    return queries


# ---- 1. boundaries: hand-made lists around the word, tile and segment ends
BOUNDARY_MAX_DOC = 131_113  # three 65 536-doc tiles; the last word holds 9 docs


@functools.lru_cache(maxsize=None)
def _boundary_segment():
    md = BOUNDARY_MAX_DOC
    a = [31, 32, 33, 63, 64, 65535, 65536, 65537, 131071, 131072, md - 1]
    lists = [a, list(range(md)), list(range(0, md, 2)), list(range(65530, 65545))]
    return O.build_segment(md, [[(d, 1) for d in l] for l in lists], [5] * md), a


@pytest.mark.parametrize("dense_ratio", [4096, 2, 1 << 16])
def test_word_tile_and_segment_boundaries(ta, dense_ratio):
    """A list has a bitmap of its own when doc_freq * dense_ratio >= max_doc: at 4096 and at 2 the short lists A and D
    are scattered into the batch's scratch, at 65 536 every list is read in place."""
    seg, a_docs = _boundary_segment()
    md = seg.max_doc
    A, B, C, D, ABSENT = 0, 1, 2, 3, 77
    queries = [(O.MODE_AND, [A, B]), (O.MODE_OR, [B]), (ta.MODE_BOOL, [C], [N]),            # MustNot only: empty
               (ta.MODE_BOOL, [B, C], [M, N]), (O.MODE_AND, [A, ABSENT]),                    # absent Must: empty
               (ta.MODE_BOOL, [A, D, C], [S, S, N]), (O.MODE_OR, [A]), (O.MODE_OR, [A, ABSENT])]
    a = np.asarray(a_docs, np.uint32)
    odd = np.arange(1, md, 2, dtype=np.uint32)
    ad = np.union1d(a, np.arange(65530, 65545, dtype=np.uint32))
    want = [a, np.arange(md, dtype=np.uint32), np.zeros(0, np.uint32), odd, np.zeros(0, np.uint32),
            ad[ad % 2 == 1].astype(np.uint32), a, a]
    # the expectations above against the oracle (where it takes the query)
    for i in (0, 1, 2, 3, 5, 6):
        assert np.array_equal(_want(seg, queries[i]), want[i]), i
    assert odd.size == 65_556 and int(odd[-1]) == 131_111
    assert want[5].tolist() == [31, 33, 63] + list(range(65531, 65544, 2)) + [131071]
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", dense_ratio)
        dev.set_option("dense_budget_x", 256)
        total = sum(w.size for w in want)
        rc, docs, starts = dev.raw_docset(queries, total, guard=8)
        assert rc == 0, ta.binding.lib().tq_last_error()
        assert int(starts[0]) == 0 and int(starts[-1]) == total
        got = _rows(docs, starts)
        _assert_rows(queries, got, want, md)
        assert got[2].size == 0 and got[4].size == 0  # empty rows between non-empty ones
        assert np.all(docs[total:] == GUARD)
        st = dev.last_batch_stats()
        assert st["kernel_mask"] == ta.binding.KERNEL_DOCSET and st["matches"] == total, st
        assert dev.last_batch_match_counts(len(queries)).tolist() == [w.size for w in want]
        n_in_place = sum(1 for t in seg.terms[:4] if t.doc_freq * dense_ratio >= md)
        assert n_in_place == (4 if dense_ratio == 1 << 16 else 2)
        assert dev.segment_stats(0)["n_dense_lists"] == n_in_place
        counts = dev.count(queries)
        assert np.diff(starts.astype(np.int64)).tolist() == counts.tolist()
    finally:
        dev.close()


# ---- 2. random parity: every flat shape, lists with and without a bitmap, with and without deletes
@pytest.mark.parametrize("seed", [31, 32])
@pytest.mark.parametrize("dense_ratio", [4096, 8])
def test_docsets_equal_the_oracle(ta, seed, dense_ratio):
    rng = np.random.default_rng(seed)
    seg = _synth(100_000 + 999 * seed, 48)
    queries = _random_queries(ta, rng, 48)
    deleted = rng.choice(seg.max_doc, size=seg.max_doc // 7, replace=False).tolist()
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", dense_ratio)
        dev.set_option("dense_budget_x", 256)
        for dels in ((), deleted):
            dev.set_alive_bitset(_alive_bytes(seg.max_doc, dels) if dels else None)
            want = [_want(seg, q, dels) for q in queries]
            got = dev.docset(queries)
            st = dev.last_batch_stats()
            assert st["kernel_mask"] == ta.binding.KERNEL_DOCSET, st
            assert all(np.all(g[:, 0] == 0) for g in got)
            _assert_rows(queries, [g[:, 1] for g in got], want, seg.max_doc)
            assert st["matches"] == sum(w.size for w in want)
            assert dev.last_batch_match_counts(len(queries)).tolist() == [w.size for w in want]
    finally:
        dev.close()


# ---- 3. capacity protocol
def test_capacity_protocol(ta):
    rng = np.random.default_rng(5)
    seg = _synth(100_000 + 999 * 31, 48)
    queries = _random_queries(ta, rng, 48)[:24]
    want = [_want(seg, q) for q in queries]
    total = sum(w.size for w in want)
    assert total > 1000
    dev = ta.DeviceIndex([seg])
    try:
        _all_dense(dev)
        rc, docs, starts = dev.raw_docset(queries, total, guard=64)
        assert rc == 0, ta.binding.lib().tq_last_error()
        _assert_rows(queries, _rows(docs, starts), want, seg.max_doc)
        assert np.all(docs[total:] == GUARD)
        for cap in (total - 1, 0):
            rc2, docs2, starts2 = dev.raw_docset(queries, cap, guard=total + 64 - cap)
            assert rc2 == ERR_INVALID
            assert ta.binding.lib().tq_last_error()
            assert np.array_equal(starts2, starts)  # complete: the caller sizes its retry from starts[n]
            assert np.all(docs2[cap:] == GUARD)     # nothing at or past cap
            rc3, docs3, starts3 = dev.raw_docset(queries, int(starts2[-1]))
            assert rc3 == 0 and np.array_equal(docs3, docs[:total]) and np.array_equal(starts3, starts)
    finally:
        dev.close()


# ---- 4. sub-batching: more lists without a bitmap than one launch scatters
def test_sub_batches_continue_the_rows(ta):
    seg = _synth(90_000, 64)
    queries = [(O.MODE_OR, [4 + i % 60, 4 + (i + 30) % 60]) for i in range(60)]
    sparse = {t for q in queries for t in q[1] if seg.terms[t].doc_freq * 8 < seg.max_doc}
    assert len(sparse) >= 40, len(sparse)
    want = [_want(seg, q) for q in queries]
    total = sum(w.size for w in want)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 8)
        dev.set_option("docset_temp_lists", 16)
        rc, docs_s, starts_s = dev.raw_docset(queries, total, guard=16)
        assert rc == 0, ta.binding.lib().tq_last_error()
        scratch_s = dev.segment_stats(0)["scratch_bytes"]
        dev.set_option("docset_temp_lists", 0)
        rc, docs_d, starts_d = dev.raw_docset(queries, total)  # default: one launch holds them all
        assert rc == 0, ta.binding.lib().tq_last_error()
        # ... in scratch bitmaps (max_doc / 8 bytes each) the sub-batched call did not need
        assert dev.segment_stats(0)["scratch_bytes"] - scratch_s >= (len(sparse) - 16) * (seg.max_doc // 8)
        _assert_rows(queries, _rows(docs_s, starts_s), want, seg.max_doc)
        assert np.array_equal(starts_s, starts_d) and np.array_equal(docs_s[:total], docs_d)
        assert np.all(docs_s[total:] == GUARD)
        assert dev.last_batch_match_counts(len(queries)).tolist() == [w.size for w in want]
        assert dev.last_batch_stats()["matches"] == total
    finally:
        dev.close()


# ---- 5. refusals: the batch fails as a whole, names the query, and the segment stays usable
def test_refusals_leave_the_segment_usable(ta):
    seg = _synth(60_000, 48, with_positions=True)
    good = [(O.MODE_AND, [0, 1]), (O.MODE_OR, [2, 40])]
    want = [_want(seg, q) for q in good]
    total = sum(w.size for w in want)
    phrase = (O.MODE_PHRASE, [0, 1], [0, 1])
    nested = (ta.MODE_BOOL, [1, 2, 3], [M, M, M], [0, 1, 1], 0, {"nested_occurs": [M, M, N]})
    bad_occur = (ta.MODE_BOOL, [1, 2], [M, 3])
    err = ta.binding.lib().tq_last_error
    dev = ta.DeviceIndex([seg])
    try:
        for bad, code in ((phrase, ERR_UNSUPPORTED), (nested, ERR_UNSUPPORTED), (bad_occur, ERR_INVALID)):
            for at in (0, 2):  # first and last of the batch
                batch = good[:at] + [bad] + good[at:]
                rc, docs, _ = dev.raw_docset(batch, total + 1000, guard=4)
                assert rc == code, (bad, rc, err())
                assert ("query %d" % at).encode() in err(), err()
                assert np.all(docs == GUARD)  # nothing was launched
                rc, docs, starts = dev.raw_docset(good, total)
                assert rc == 0, err()
                _assert_rows(good, _rows(docs, starts), want, seg.max_doc)
    finally:
        dev.close()


# ---- 6. device outputs
def test_device_variant(ta):
    import torch

    rng = np.random.default_rng(9)
    seg = _synth(100_000 + 999 * 32, 48)
    queries = _random_queries(ta, rng, 48)[10:40]
    deleted = rng.choice(seg.max_doc, size=seg.max_doc // 7, replace=False).tolist()
    want = [_want(seg, q, deleted) for q in queries]
    flat = np.concatenate(want)
    total, n = flat.size, len(queries)
    want_starts = np.concatenate([[0], np.cumsum([w.size for w in want])]).astype(np.int64)
    dev = ta.DeviceIndex([seg])
    try:
        dev.set_option("dense_ratio", 8)
        dev.set_alive_bitset(_alive_bytes(seg.max_doc, deleted))
        guard32 = np.array([GUARD], np.uint32).view(np.int32)[0]
        for cap in (total // 2, total):
            dev.set_option("docset_temp_lists", 0 if cap < total else 16)  # (the full run: in sub-batches)
            d_docs = torch.full((total + 64,), int(guard32), dtype=torch.int32, device="cuda")
            d_starts = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            rc = dev.raw_docset_device(queries, d_docs, cap, d_starts)
            assert rc == 0, ta.binding.lib().tq_last_error()
            st = dev.last_batch_stats()  # (waits for the batch)
            torch.cuda.synchronize()
            docs = d_docs.cpu().numpy().view(np.uint32)
            starts = d_starts.cpu().numpy()
            assert np.array_equal(starts, want_starts)  # the full total, whatever the capacity
            assert np.array_equal(docs[:cap], flat[:cap])
            assert np.all(docs[cap:] == GUARD)
            assert st["kernel_mask"] == ta.binding.KERNEL_DOCSET and st["matches"] == total, st
    finally:
        dev.close()


# ---- 7. host mirror over two segments
def test_host_mirror_over_two_segments(ta):
    rng = np.random.default_rng(13)
    segs = [_synth(70_000, 48, 0), _synth(83_001, 48, 1)]
    queries = _random_queries(ta, rng, 48)
    deleted = rng.choice(segs[1].max_doc, size=segs[1].max_doc // 5, replace=False).tolist()
    dev = ta.DeviceIndex(segs)
    try:
        dev.set_option("dense_ratio", 8)
        dev.set_alive_bitset(_alive_bytes(segs[1].max_doc, deleted), segment_ord=1)
        got = dev.docset(queries)
        for q, g in zip(queries, got):
            w0, w1 = _want(segs[0], q), _want(segs[1], q, deleted)
            want = np.concatenate([np.stack([np.zeros_like(w0), w0], axis=1), np.stack([np.ones_like(w1), w1], axis=1)])
            assert g.dtype == np.uint32 and g.shape == want.shape and np.array_equal(g, want), q
        assert np.array_equal(dev.count(queries), np.array([g.shape[0] for g in got], np.uint64))
    finally:
        dev.close()
