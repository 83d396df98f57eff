"""The crafted segments of the term-preparation table tests (tests/test_prepare_model_cpu.py without a GPU,
tests/test_gpu_prepare_tables.py on one): every list is placed so that a builder's edge is hit — see each case's
comment.  Built once per module by the tests' fixtures and never changed."""
import numpy as np

from oracle import oracle as O

MAX_DOC_A = 300_007      # odd, above 2^18: every range-maxima level has two live entries, every last word / range partial
MAX_DOC_B = 4_099        # the smallest segment that may get range directories (rdir_plan's floor is 4 096)
MAX_DOC_C = 16_842_829   # 257 * 65 536 + 77: 258 scan tiles of the rank directory — td_scan_tiles_kernel's second chunk
DENSE_RATIO_A, DENSE_RATIO_B, DENSE_RATIO_C = 1024, 4, 8192  # lists from 293 / 1 025 / 2 057 postings get tables of their own
EDGE_TFS = [1, 2, 3, 254, 255, 256, 65_534, 65_535, 65_536]  # the tf8, tf-class and rdir-entry saturations
AVG_TOKENS = 19          # total_num_tokens = 19 * max_doc: norms of the order of the tfs, t spread over (0, 1), few 255 t on an integer


class Case:
    def __init__(self, name, max_doc, lists, notes, fieldnorm_ids, dense_ratio, with_positions=True, basic=False):
        self.name, self.max_doc, self.lists, self.notes, self.dense_ratio = name, max_doc, lists, notes, dense_ratio
        self.fieldnorm_ids = fieldnorm_ids
        self.with_positions = with_positions
        self.record_option = O.BASIC if basic else (O.WITH_FREQS_AND_POSITIONS if with_positions else O.WITH_FREQS)
        self.has_freq = not basic
        fieldnorms = None if fieldnorm_ids is None else np.asarray(O.fieldnorm_table(), np.int64)[fieldnorm_ids].tolist()
        # (positions: 0 .. tf - 1 of every posting — the tables only count them)
        positions = [[range(tf) for _, tf in pl] for pl in lists] if with_positions else None
        self.seg = O.build_segment(max_doc, lists, fieldnorms, record_option=self.record_option, positions=positions,
                                   total_num_tokens=AVG_TOKENS * max_doc)
        if fieldnorm_ids is not None:
            assert np.array_equal(self.seg.fieldnorm, fieldnorm_ids.astype(np.uint8))

    @classmethod
    def wrap(cls, name, seg, lists, fieldnorm_ids, dense_ratio, with_positions):
        """A segment built elsewhere, whose lists are known, as a Case."""
        c = cls.__new__(cls)
        c.name, c.max_doc, c.lists, c.notes, c.dense_ratio = name, seg.max_doc, lists, [""] * len(lists), dense_ratio
        c.fieldnorm_ids = None if fieldnorm_ids is None else np.asarray(fieldnorm_ids, np.int64)
        c.with_positions, c.record_option, c.has_freq, c.seg = with_positions, seg.record_option, seg.record_option != O.BASIC, seg
        return c

    def is_dense(self, t):
        return self.max_doc >= 4096 and len(self.lists[t]) * self.dense_ratio >= self.max_doc

    def by_note(self, word):
        return [t for t, n in enumerate(self.notes) if word in n]


def _fieldnorm_ids(rng, max_doc):
    """mostly short docs, one doc in 32 from the whole id range (the longest docs have t below 1e-6: a byte boundary by the 1e-4 rule), ids 0 and 255 at both ends of the segment"""
    ids = rng.integers(1, 41, size=max_doc)
    wild = rng.random(max_doc) < 1 / 32
    ids[wild] = rng.integers(0, 256, size=int(wild.sum()))
    ids[[0, max_doc - 1]] = [255, 0]
    ids[[1, max_doc - 2]] = [0, 255]
    return ids.astype(np.int64)


def _tfs(rng, n, edge=False):
    tfs = rng.choice([1, 1, 1, 2, 2, 3, 4, 7], size=n)
    if edge:  # every edge tf, scattered; three of them next to each other
        at = rng.choice(n, size=min(n, len(EDGE_TFS)), replace=False)
        tfs[at] = EDGE_TFS[:len(at)]
    return tfs.astype(np.int64)


def _spread(rng, max_doc, df, lo=0, hi=None, edge=False):
    docs = np.sort(rng.choice(np.arange(lo, max_doc if hi is None else hi), size=df, replace=False))
    return list(zip(docs.tolist(), _tfs(rng, df, edge).tolist()))


def shaped_case(name, max_doc, dense_ratio, lengths, runs_at, n_columns, n_sparse, seed):
    """lengths: the list lengths around the 128-posting block and the device walk's rounds of 64 skip entries; runs_at:
    (k1, k2) — the 1024-doc ranges whose first doc the run list reaches at posting 64 and at posting 256."""
    rng = np.random.default_rng(seed)
    fn = _fieldnorm_ids(rng, max_doc)
    dense_df = -(-max_doc // dense_ratio)
    lists, notes = [], []

    def add(pl, note):
        lists.append(pl)
        notes.append(note)

    for df in lengths:
        add(_spread(rng, max_doc, df, edge=df >= 127), "length %d" % df)
    # the segment's ends
    add(_spread(rng, max_doc - 1, dense_df + 7) + [(max_doc - 1, 255)], "last doc dense")
    add([(0, 256)] + _spread(rng, max_doc, dense_df + 7, lo=1), "first doc dense")
    add(_spread(rng, max_doc - 1, 279) + [(max_doc - 1, 3)], "last doc rdir")
    add([(0, 2)] + _spread(rng, max_doc, 279, lo=1), "first doc rdir")
    # a run of consecutive docs over a 1024-doc boundary at posting 63 -> 64 (two wavefronts) and at 255 -> 256 (two
    # workgroups of td_rmax_scatter_kernel), the larger tf on either side of a boundary in turn
    k1, k2 = runs_at
    docs = list(range(1024 * k1 - 64, 1024 * k1 + 64)) + list(range(1024 * k2 - 128, 1024 * k2 + 128))
    extra = max(0, dense_df - len(docs))
    docs += np.sort(rng.choice(np.arange(1024 * k2 + 200, max_doc), size=extra, replace=False)).tolist()
    tfs = _tfs(rng, len(docs))
    tfs[[63, 64, 255, 256]] = [9, 1, 1, 9]
    add(list(zip(docs, tfs.tolist())), "runs dense")
    # several empty directory ranges in a row, then ranges full of postings, then empty ranges to the end
    lo = max_doc * 2 // 3
    docs = [3, 5] + list(range(lo, lo + 270)) + [lo + 400]
    add(list(zip(docs, _tfs(rng, len(docs), edge=True).tolist())), "gaps rdir")
    add([(d, 1) for d, _ in _spread(rng, max_doc, dense_df + 40)], "tf one dense")
    add([(d, 1) for d, _ in _spread(rng, max_doc, 280)], "tf one rdir")
    # more dense lists than the doc matrix has columns, more lists without a column than there are signature bits
    for i in range(n_columns):
        add(_spread(rng, max_doc, dense_df + int(rng.integers(0, 30)), edge=i % 7 == 0), "column %d dense" % i)
    for i in range(n_sparse):
        add(_spread(rng, max_doc, int(rng.integers(1, 60))), "sparse %d" % i)
    for pl, note in zip(lists, notes):
        assert ("dense" in note) == (len(pl) * dense_ratio >= max_doc) or note.startswith(("length", "sparse")), (note, len(pl))
        assert "rdir" not in note or (256 <= len(pl) and len(pl) * dense_ratio < max_doc), (note, len(pl))
    return Case(name, max_doc, lists, notes, fn, dense_ratio)


LENGTHS_A = [1, 127, 128, 129, 255, 256, 257, 64 * 128, 64 * 128 + 1, 65 * 128 + 77, 8192 + 5]
LENGTHS_B = [1, 127, 128, 129, 255, 256, 257, 1024, 1025, 2000]


def case_a():
    return shaped_case("A", MAX_DOC_A, DENSE_RATIO_A, LENGTHS_A, (3, 9), 44, 40, seed=7001)


def case_b():
    return shaped_case("B", MAX_DOC_B, DENSE_RATIO_B, LENGTHS_B, (1, 2), 0, 24, seed=7002)


def case_c():
    """Three lists of 2 000 to 3 000 postings, no fieldnorm file (the constant id), no positions: docs around the
    multiples of 65 536 words' tiles (2 048 bitmap words = 65 536 docs per scan tile), around word 256 * 2 048 — where the
    one workgroup that scans the tile sums starts its second chunk of 256 tiles and has to carry — and in the last word."""
    rng = np.random.default_rng(7003)
    lists = []
    tile_docs = 65_536
    for li, df in enumerate((2100, 2600, 3000)):
        docs = set([MAX_DOC_C - 1, MAX_DOC_C - 1 - li, 256 * tile_docs - 1, 256 * tile_docs, 256 * tile_docs + 31 + li])
        for tile in list(range(1, 258, 37 + li)) + [255, 256, 257]:
            lo, hi = tile * tile_docs - 100, min(MAX_DOC_C, tile * tile_docs + 100)
            docs.update(rng.choice(np.arange(lo, hi), size=min(60, hi - lo), replace=False).tolist())
        docs.update(range(MAX_DOC_C - 40, MAX_DOC_C, 3))
        assert len(docs) < df
        while len(docs) < df:
            docs.add(int(rng.integers(0, MAX_DOC_C)))
        docs = sorted(docs)
        lists.append(list(zip(docs, _tfs(rng, len(docs), edge=True).tolist())))
    return Case("C", MAX_DOC_C, lists, ["tiles dense"] * 3, None, DENSE_RATIO_C, with_positions=False)


def case_basic():
    """BASIC records (TqdTermHead::has_freq bit 0 clear, every tf reads as 1) on segment B's doc space: a list with a
    range directory, a dense list with a one-posting tail, a list of one vint block."""
    rng = np.random.default_rng(7004)
    fn = _fieldnorm_ids(rng, MAX_DOC_B)
    lists = [[(d, 1) for d, _ in _spread(rng, MAX_DOC_B, df)] for df in (300, 1025, 90)]
    return Case("basic", MAX_DOC_B, lists, ["basic rdir", "basic dense", "basic sparse"], fn, DENSE_RATIO_B,
                with_positions=False, basic=True)
