"""The shared intersections' warm-up tasks inside the main dispatch (option "ashare_inline_warm"): 2 000 Zipf pairs over a
1M-doc segment of 256 lists, k = 10 — the smallest shape whose leaders come both with and without warm-up tasks
(tests/test_ashare_order_cpu.py checks that on the planner).  One dispatch (2), two dispatches (0) and the rule (1) return
the same rows, and those are the exhaustive mode's: thresholds are advisory, a dependent task that starts before its
leader's warm-up tasks have ended only prunes less."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu


def test_one_dispatch_equals_two_and_the_exhaustive_mode():
    import tantivy_amd

    seg = O.synth_segment(1_000_000, n_terms=256)
    queries = [(O.MODE_AND, t.tolist()) for t in O.zipf_queries(2000, 2, 256, seed=21)]
    dev = tantivy_amd.DeviceIndex([seg], devices=[0])
    try:
        dev.set_option("exhaustive", 1)
        want = dev.search(queries, 10)
        dev.set_option("exhaustive", 0)
        got = {}
        for mode in (0, 2, 1):
            dev.set_option("ashare_inline_warm", mode)
            got[mode] = dev.search(queries, 10)
            assert "ashare" in dev.last_batch_stats()["kernels"], (mode, dev.last_batch_stats())
        for mode in (0, 2, 1):
            for name, w, g in zip(("scores", "segment_ords", "docs", "counts"), want, got[mode]):
                assert np.array_equal(np.asarray(w).view(np.uint32), np.asarray(g).view(np.uint32)), (mode, name)
    finally:
        dev.close()
