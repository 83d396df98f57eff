"""Searcher::search on the device as one native call (tqh_search_prepared_device) against the path it replaces for one
rank: collect_segment per segment (tqh_collect_segment_prepared_device) + merge_top_k (tq_merge_topk_device).  The four
arrays — scores, segment ordinals, docs, counts — must be the same raw bits, for an index of one segment (the segment's
merge kernels write the rows and the ordinal column themselves, no merge_top_k launch) and of two (collects + one
merge launch inside the call), for both instantiations of the top-k registers (k = 10 and k = 100), pruned and
exhaustive, into pinned host memory and into plain device memory."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

N_TERMS = 64
ABSENT = N_TERMS + 5  # a term id no segment has a TermInfo for


def _batch():
    """~600 queries: 2-term ANDs of a Zipf stream with repeats (twins inside a leader's group, out_index), 3-term ORs,
    one-term queries, an AND with an absent term, ANDs of the rarest lists (fewer than k matches)."""
    a = O.zipf_queries(300, 2, N_TERMS, seed=11)
    o = O.zipf_queries(120, 3, N_TERMS, seed=12)
    qs = [(O.MODE_AND, t.tolist()) for t in a]
    qs += [(O.MODE_AND, a[i].tolist()) for i in range(0, 300, 3)]  # repeated queries
    qs += [(O.MODE_OR, t.tolist()) for t in o]
    qs += [(O.MODE_OR, [t]) for t in (0, 1, 7, 31, 62, 63)] * 5
    qs += [(O.MODE_AND, [3, ABSENT]), (O.MODE_AND, [ABSENT, 0])]
    qs += [(O.MODE_AND, [62, 63]), (O.MODE_AND, [61, 63]), (O.MODE_AND, [59, 62, 63]), (O.MODE_AND, [60, 61, 62, 63])] * 4
    rng = np.random.default_rng(3)
    return [qs[i] for i in rng.permutation(len(qs))]


@pytest.fixture(scope="module")
def indexes():
    """The two indexes every case shares: one segment of 50 000 docs, two of 25 000."""
    return {1: [O.synth_segment(50_000, n_terms=N_TERMS)],
            2: [O.synth_segment(25_000, n_terms=N_TERMS, segment_ord=o) for o in range(2)]}


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _both_paths(segs, k, exhaustive, device_out):
    import torch

    import tantivy_amd
    from tantivy_amd import distributed as D

    queries = _batch()
    n, S = len(queries), len(segs)
    cuda = torch.device("cuda", 0)
    dev = tantivy_amd.DeviceIndex(segs, devices=[0] * S)
    stream = torch.cuda.Stream(device=cuda)
    try:
        dev.set_option("ashare_min_batch", 1)
        dev.set_option("exhaustive", exhaustive)
        dev.prepare(queries)
        slabs = (torch.empty((S * n, k), dtype=torch.float32, device=cuda),
                 torch.empty((S * n, k), dtype=torch.int32, device=cuda),
                 torch.empty(S * n, dtype=torch.int32, device=cuda))

        def rows():  # (filled with a pattern: a slot the call leaves unwritten shows)
            ts = [torch.full(shape, 0x5A5A5A5A, dtype=torch.int32) for shape in ((n, k), (n, k), (n, k), (n,))]
            ts[0] = ts[0].view(torch.float32)
            return [t.to(cuda) if device_out else t.pin_memory() for t in ts]

        # the two-kernel path: collect_segment per segment into the slabs, then merge_top_k
        for s in range(S):
            dev.collect_segment_prepared_device(s, k, slabs[0][s * n:(s + 1) * n], slabs[1][s * n:(s + 1) * n],
                                                slabs[2][s * n:(s + 1) * n], stream.cuda_stream)
        want = rows()
        D.merge_gathered_device(dev.ctx, 0, slabs[0].view(S, n, k), slabs[1].view(S, n, k), slabs[2].view(S, n), 0, k,
                                stream.cuda_stream, out=tuple(want))
        stream.synchronize()
        want = [_bits(t).copy() for t in want]
        for t in slabs:
            t.fill_(-1)
        # the one call
        got = rows()
        dev.search_prepared_device(k, got, slabs if S > 1 else None, stream.cuda_stream)
        stream.synchronize()
        kernels = dev.last_batch_stats()["kernels"]
        merge_ms = dev.exchange_ms()
        return queries, want, [_bits(t).copy() for t in got], kernels, merge_ms
    finally:
        dev.close()


@pytest.mark.parametrize("k,exhaustive", [(10, 0), (10, 1), (100, 0), (100, 1)])
@pytest.mark.parametrize("n_segments", [1, 2])
def test_one_call_rows_equal_the_two_kernel_path_bit_for_bit(indexes, n_segments, k, exhaustive):
    queries, want, got, kernels, merge_ms = _both_paths(indexes[n_segments], k, exhaustive, device_out=False)
    for name, w, g in zip(("scores", "segment_ords", "docs", "counts"), want, got):
        assert np.array_equal(w, g), (name, np.argwhere(w != g)[:5])
    counts = want[3]
    absent = [i for i, q in enumerate(queries) if ABSENT in q[1]]
    assert absent and all(counts[i] == 0 for i in absent)
    assert np.any((counts > 0) & (counts < k)), "no query with fewer than k matches in the batch"
    assert np.all(want[1][counts == 0] == 0xFFFFFFFF)  # (an empty row's ordinals are all padding)
    if not exhaustive:
        assert "ashare" in kernels, kernels  # the shared intersection launch ran (merge_lists_kernel's epilogue)
    # one segment merges nothing; two ran exactly the merge launch the events stand around
    assert (merge_ms == 0.0) if n_segments == 1 else (merge_ms > 0.0)


def test_one_call_into_plain_device_tensors(indexes):
    _, want, got, _, _ = _both_paths(indexes[1], 10, 0, device_out=True)
    for name, w, g in zip(("scores", "segment_ords", "docs", "counts"), want, got):
        assert np.array_equal(w, g), (name, np.argwhere(w != g)[:5])


def test_shard_runner_takes_the_one_call_and_reports_no_exchange(indexes):
    """ShardRunner.enqueue with one rank: same results as Searcher::search on the host path, exchange_ms() == 0.0 for the
    index of one segment (no exchange, no merge launch), > 0 for two local segments (the call's own merge launch)."""
    import tantivy_amd
    from tantivy_amd import distributed as D

    queries = _batch()
    for n_segments in (1, 2):
        segs = indexes[n_segments]
        dev = tantivy_amd.DeviceIndex(segs, devices=[0] * n_segments)
        try:
            dev.set_option("ashare_min_batch", 1)
            want = dev.search(queries, 10)
        finally:
            dev.close()
        run = D.ShardRunner(segs, 0)
        try:
            run.set_option("ashare_min_batch", 1)
            run.prepare(queries, 10)
            for _ in range(2):
                run.enqueue()
            run.synchronize()
            got = run.results()
            for w, g in zip(want, got):
                assert np.array_equal(np.asarray(w).view(np.uint32), np.asarray(g).view(np.uint32))
            ms = run.exchange_ms()
            assert (ms == 0.0) if n_segments == 1 else (ms > 0.0)
        finally:
            run.close()
