"""The numpy models of the derived tables (tests/prepare_model.py) without a GPU, on the crafted segments the device
is compared with (tests/prepare_cases.py): block records, tails and coarse table against what the host walker leaves
(tools/planbench/walk_check.cpp), rank words against a cumulative sum of popcounts, range directories by answering "is d
in the list, with which tf" for every doc from the model's tables alone, range maxima by their soundness at every level —
and the cases themselves: how many postings sit where an f32 divide may round a range-maximum byte the other way."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import prepare_cases as PC
from tests import prepare_model as PM
from tests.test_term_walk_cpu import run_walk, walk_check  # noqa: F401  (walk_check: the fixture that builds the tool)


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in (PC.case_a(), PC.case_b(), PC.case_c())}


def local_cache(case):
    """Bm25Weight.cache under the segment's own average fieldnorm, as the oracle computes it (the device test reads the
    segment's copy back instead)"""
    avg = float(np.float32(case.seg.total_num_tokens) / np.float32(case.max_doc))
    return np.array(list(O.bm25_for_one_term(1, case.max_doc, avg).cache), np.float32)


def test_the_cases_hold_what_they_are_for(cases):
    a, b, c = cases["A"], cases["B"], cases["C"]
    for case in (a, b):
        lens = [len(pl) for pl in case.lists]
        assert {1, 127, 128, 129, 255, 256, 257} <= set(lens)
        assert any(pl[-1][0] == case.max_doc - 1 for pl in case.lists) and any(pl[0][0] == 0 for pl in case.lists)
        assert {0, 255} <= set(case.fieldnorm_ids.tolist())
        tfs = {tf for pl in case.lists for _, tf in pl}
        assert set(PC.EDGE_TFS) <= tfs
        (runs,) = case.by_note("runs")
        docs = [d for d, _ in case.lists[runs]]
        assert docs[64] % 1024 == 0 and docs[63] == docs[64] - 1 and docs[256] % 1024 == 0 and docs[255] == docs[256] - 1
        for t in case.by_note("rdir"):
            assert PM.rdir_shift(case.max_doc, len(case.lists[t])) > 0
    assert {64 * 128, 64 * 128 + 1, 65 * 128 + 77, 8192 + 5} <= {len(pl) for pl in a.lists}
    n_dense = sum(a.is_dense(t) for t in range(len(a.lists)))
    assert n_dense > PM.MAT_SLOTS and len(a.lists) - PM.MAT_SLOTS > PM.SIG_BITS + PM.MAT_SLOTS
    for l in range(PM.RM_LEVELS):  # two live entries at every level, a partial group of four at every pooling
        assert (a.max_doc >> (PM.RM_SHIFT + 2 * l)) >= 1
    # C: more scan tiles of 2 048 bitmap words than one chunk of 256 — postings on both sides of the chunk boundary
    assert PM.bitmap_words(c.max_doc) > 256 * 2048
    for pl in c.lists:
        docs = PM.arrays(pl)[0]
        assert 2000 <= len(pl) <= 3000 and docs[-1] == c.max_doc - 1
        assert ((docs >> 5) < 256 * 2048).any() and ((docs >> 5) >= 256 * 2048).sum() > 60
        assert all(c.is_dense(t) for t in range(len(c.lists)))


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_records_tails_and_coarse_table_against_the_host_walk(walk_check, tmp_path, cases, name):  # noqa: F811
    case = cases[name]
    walked = run_walk(walk_check, tmp_path, case.seg)
    for t, (pl, w) in enumerate(zip(case.lists, walked)):
        assert w["ok"], w
        rec = PM.rec(pl, case.seg.postings_bytes(t), case.record_option, case.with_positions)
        assert w["n_blocks"] == len(rec) - 1
        assert w["rec"] == rec[:-1].tolist(), (name, t)
        assert rec[-1].tolist() == [PM.TERMINATED, 0, 0, w["n_positions"]]
        tail_docs, tail_tfs = PM.tails(pl)
        assert w["tail_docs"] == tail_docs.tolist() and w["tail_tfs"] == tail_tfs.tolist(), (name, t)
        shift, coarse = PM.coarse(case.max_doc, pl)
        assert w["shift"] == shift and w["coarse"] == coarse.tolist(), (name, t)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_rank_words_are_the_running_popcount(cases, name):
    case = cases[name]
    for t, pl in enumerate(case.lists):
        if not case.is_dense(t) and t % 5:
            continue
        d = PM.dense(case.max_doc, pl)
        assert len(d) == (case.max_doc + 31) // 32 + 1
        pop = np.array([bin(int(x)).count("1") for x in d[:, 0][d[:, 0] != 0]])
        full = np.zeros(len(d), np.int64)
        full[d[:, 0] != 0] = pop
        assert np.array_equal(d[:, 1], np.cumsum(full) - full)
        assert full.sum() == len(pl) and not d[(case.max_doc + 31) // 32:, 0].any()
        b = PM.bits(case.max_doc, pl)
        assert len(b) % 256 == 0 and np.array_equal(b[:len(d)], d[:, 0]) and not b[len(d):].any()
        pd = PM.pos_dir(pl)
        tfs = [tf for _, tf in pl]
        assert len(pd) == (len(pl) + 3) // 4 + 1 and pd[-1] == sum(tfs)
        assert pd.tolist() == [sum(tfs[:4 * j]) for j in range(len(pd))]


@pytest.mark.parametrize("name", ["A", "B"])
def test_range_directories_answer_for_every_doc(cases, name):
    case = cases[name]
    checked = 0
    for t, pl in enumerate(case.lists):
        S = PM.rdir_shift(case.max_doc, len(pl))
        if not S or case.is_dense(t):
            continue
        checked += 1
        directory, entries = PM.rdir(case.max_doc, pl, S)
        assert len(directory) == (case.max_doc >> S) + 2 and directory[0] == 0 and directory[-1] == len(pl)
        assert (case.max_doc >> S) + 1 <= len(pl) and (S == 2 or (case.max_doc >> (S - 1)) + 1 > len(pl))
        # every d in [0, max_doc): walk the entries of d's range, vectorised over the docs
        d = np.arange(case.max_doc, dtype=np.int64)
        lo, hi = directory[d >> S], directory[(d >> S) + 1]
        got = np.zeros(case.max_doc, np.int64)
        k = 0
        while True:
            live = np.nonzero(lo + k < hi)[0]
            if not len(live):
                break
            e = entries[lo[live] + k]
            hit = (e >> 16) == (live & ((1 << S) - 1))
            got[live[hit]] = e[hit] & 0xFFFF
            k += 1
        want = np.zeros(case.max_doc, np.int64)
        docs, tfs = PM.arrays(pl)
        want[docs] = np.minimum(tfs, 0xFFFF)
        assert np.array_equal(got, want), (name, t)
        for doc in (0, int(docs[0]), int(docs[-1]), case.max_doc - 1):  # ... and the scalar form the device test words it in
            assert PM.rdir_lookup(case.max_doc, directory, entries, S, doc) == want[doc]
    assert checked >= 4


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_range_maxima_are_sound_at_every_level(cases, name):
    case = cases[name]
    cache = local_cache(case)
    n_postings = n_near = 0
    for t, pl in enumerate(case.lists):
        docs, _ = PM.arrays(pl)
        tt = PM.rmax_t(pl, case.fieldnorm_ids, 1, cache)
        levels, lmax = PM.rmax(case.max_doc, pl, case.fieldnorm_ids, 1, cache)
        assert lmax == levels[0].max() and 1 <= lmax <= 255
        for l, lv in enumerate(levels):
            assert len(lv) == PM.rm_level_entries(case.max_doc, l) and len(lv) % 4 == 0
            # q / 255 >= t for every posting, in the one entry of the level its doc can touch
            q = lv[docs >> (PM.RM_SHIFT + 2 * l)]
            assert (q / 255.0 >= tt).all(), (name, t, l)
            live = (case.max_doc >> (PM.RM_SHIFT + 2 * l)) + 1
            assert not lv[live:].any()  # the padding
            # tight: no entry above the byte of the largest t below it
            want = np.zeros(len(lv), np.int64)
            np.maximum.at(want, docs >> (PM.RM_SHIFT + 2 * l), PM.rmax_byte(tt))
            assert np.array_equal(lv, want), (name, t, l)
        n_postings += len(pl)
        n_near += int(PM.rmax_near_integer(tt).sum())
    # the device divides in f32: a byte may differ by one only where 255 t lies within 1e-4 of an integer — the cases
    # keep such postings under 1 % (tests/test_gpu_prepare_tables.py asserts the same of the read-back cache)
    print("%s: %d of %d postings within 1e-4 of a byte boundary" % (name, n_near, n_postings))
    assert n_near * 100 < n_postings, (n_near, n_postings)


def test_matrices_lnorm_and_flat_on_a_hand_made_list():
    pl_a, pl_b, pl_c = [(0, 1), (5, 2), (9, 3)], [(5, 7), (6, 1)], [(9, 300)]
    fn = np.arange(10, dtype=np.int64) + 20
    m = PM.docmat(10, fn, 1, {0: pl_a, 39: pl_b}, [(15, pl_c), (15, pl_b), (0, pl_a)])
    assert m[5] == 25 | 1 << 8 | 1 << 47 | 1 << 63 | 1 << 48 and m[1] == 21 and m[9] == 29 | 1 << 8 | 1 << 63 | 1 << 48
    c = PM.doccls(10, {0: pl_a, 31: pl_b, 32: pl_c})
    assert c[0] == 1 and c[5] == 2 | 3 << 62 and c[6] == 1 << 62 and c[9] == 3
    assert PM.docmat(3, None, 1, {}, []).tolist() == [1, 1, 1]
    ln = PM.lnorm(pl_a, fn)
    assert len(ln) == 128 and ln[:3].tolist() == [20, 25, 29] and not ln[3:].any()
    docs, off, tf8 = PM.flat(pl_c + [(11, 2)])
    assert off == 16 and docs.tolist() == [9, 11] and tf8.tolist() == [255, 2]
