"""Term preparation's derived tables, read back (tq_term_table_read / tq_term_table_info) and compared with the numpy
models of tests/prepare_model.py on the crafted segments of tests/prepare_cases.py — through every builder that is only
assumed to agree with the others: tq_term_prepare with the host walk and with the device walk, tq_term_prepare_batch
(docsig_batch_kernel's directory builder), both "use_dpp" settings of the decode that feeds the builders, the probe
pool's tables, the leader norms and the plain arrays; then the doc matrix and the tf classes after a rejected list, a
released term set and evicted probe slots, and a list of a non-primary field.

Everything is compared for EXACT equality: these are integers and bit masks.  The one exception is the range-maximum
bytes, where the device divides in f32: f32 division and multiplication are correctly rounded, each within 2^-24
relative, so 255 t computed in f32 lies within a few units of 255 * 2^-24 = 1.5e-5 of its float64 value — under 1e-4.  A
byte may therefore differ from the model by one only where the model's 255 t lies within 1e-4 of an integer; such
postings stay under 1 % of a case's postings (asserted here for the read-back cache, in tests/test_prepare_model_cpu.py
for the oracle's), and the soundness inequality q / 255 >= t is asserted of every posting at every level, no exception.

Not reached here: the tile scan's second chunk for POSITION directories, which takes a list of more than two million
postings (test_full_size_phrase of tests/test_gpu_parity.py prepares one and the preparation checks the directory's
total); segment C reaches that chunk for the rank directory, which runs the same td_scan_tiles_kernel."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import prepare_cases as PC
from tests import prepare_model as PM

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
TQ_ERR_FORMAT = 3
M, S_, N = O.MUST, O.SHOULD, O.MUST_NOT
PATHS = [("host", 1), ("device", 1), ("batch", 1), ("host", 0), ("batch", 0)]


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


class World:
    """A case and the models of its lists, computed once (under the segment's cache as the oracle computes it; every
    test first asserts that the device's copy holds exactly those floats)."""

    def __init__(self, case):
        self.case = case
        avg = float(np.float32(case.seg.total_num_tokens) / np.float32(case.max_doc))
        self.cache = np.array(list(O.bm25_for_one_term(1, case.max_doc, avg).cache), np.float32)
        self.const_id = 1  # FieldNormReader::constant(max_doc, 1)
        self._m = {}

    def model(self, t, name):
        key = (t, name)
        if key not in self._m:
            c, pl = self.case, self.case.lists[t]
            if name == "rec":
                v = PM.rec(pl, c.seg.postings_bytes(t), c.record_option, c.with_positions)
            elif name == "coarse":
                v = PM.coarse(c.max_doc, pl)
            elif name == "dense":
                v = PM.dense(c.max_doc, pl)
            elif name == "t":
                v = PM.rmax_t(pl, c.fieldnorm_ids, self.const_id, self.cache)
            self._m[key] = v
        return self._m[key]


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(name):
        if name not in made:
            made[name] = World({"A": PC.case_a, "B": PC.case_b, "C": PC.case_c, "basic": PC.case_basic}[name]())
        return made[name]

    return get


# ---------------------------------------------------------------- preparing through the raw C ABI
def _infos(ta, seg, ids):
    arr = (ta.binding.TqTermInfo * max(1, len(ids)))()
    for i, t in enumerate(ids):
        ti = seg.terms[t]
        arr[i].postings_off, arr[i].postings_len = ti.postings_start, ti.postings_end - ti.postings_start
        arr[i].positions_off, arr[i].positions_len = ti.positions_start, ti.positions_end - ti.positions_start
        arr[i].doc_freq = ti.doc_freq
    return arr


def _prepare_one_rc(ta, dev, seg, t):
    ti = seg.terms[t]
    h = C.c_uint32(NONE)
    rc = ta.binding.lib().tq_term_prepare(dev.segment_raw(), ti.postings_start, ti.postings_end - ti.postings_start,
                                          ti.positions_start, ti.positions_end - ti.positions_start, ti.doc_freq, C.byref(h))
    return rc, int(h.value)


def _prepare_one(ta, dev, seg, t):
    rc, h = _prepare_one_rc(ta, dev, seg, t)
    assert rc == 0, ta.binding.lib().tq_last_error()
    return h


def _prepare(ta, dev, seg, ids, path):
    if path == "batch":
        out = np.full(max(1, len(ids)), NONE, np.uint32)
        rc = ta.binding.lib().tq_term_prepare_batch(dev.segment_raw(), _infos(ta, seg, ids), len(ids), ta.binding._u32(out))
        assert rc == 0, ta.binding.lib().tq_last_error()
        return out[:len(ids)].tolist()
    dev.set_option("device_prepare", 1 if path == "device" else 0)
    return [_prepare_one(ta, dev, seg, t) for t in ids]


def _open(ta, case, use_dpp=1, **opts):
    dev = ta.DeviceIndex([case.seg])
    dev.set_option("dense_ratio", case.dense_ratio)
    dev.set_option("dense_budget_x", 64)  # (the matrices of a segment this small outweigh its index many times)
    dev.set_option("use_dpp", use_dpp)
    for k, v in opts.items():
        dev.set_option(k, v)
    return dev


# ---------------------------------------------------------------- comparisons
def _eq(got, want, what):
    got, want = np.asarray(got).astype(np.int64).ravel(), np.asarray(want).astype(np.int64).ravel()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = np.nonzero(got != want)[0]
        raise AssertionError("%s: %d of %d differ, first at %d: got %d, want %d" % (what, len(at), len(got), at[0], got[at[0]], want[at[0]]))


def _slot_bit(info):
    hf = info["has_freq"]
    return ((hf >> 8) & 0xFF) - 1, ((hf >> 16) & 0xFF) - 1, bool(hf >> 24 & 1)


def check_rmax(world, t, table, rmax_list, what):
    """The range-maxima table of list t (every level) and the list's maximum: sound without exception, the documented
    byte except at most one off where 255 t is within 1e-4 of an integer, every level the pooling of the level below,
    every padding entry 0.  -> (postings within 1e-4 of an integer, postings)"""
    c = world.case
    docs, _ = PM.arrays(c.lists[t])
    tt = world.model(t, "t")
    byte, near = PM.rmax_byte(tt), PM.rmax_near_integer(tt).astype(np.int64)
    assert len(table) == PM.rm_level_off(c.max_doc, PM.RM_LEVELS), (what, len(table))
    levels = [table[PM.rm_level_off(c.max_doc, l): PM.rm_level_off(c.max_doc, l + 1)].astype(np.int64) for l in range(PM.RM_LEVELS)]
    for l, lv in enumerate(levels):
        r = docs >> (PM.RM_SHIFT + 2 * l)
        assert (lv[r] / 255.0 >= tt).all(), "%s: level %d is not a bound of posting %d" % (what, l, int(np.argmin(lv[r] / 255.0 - tt)))
        lo, hi = np.zeros(len(lv), np.int64), np.zeros(len(lv), np.int64)
        np.maximum.at(lo, r, byte - near)
        np.maximum.at(hi, r, np.minimum(255, byte + near))
        bad = np.nonzero((lv < lo) | (lv > hi))[0]
        assert not len(bad), "%s: level %d entry %d holds %d, the model %d..%d" % (what, l, bad[0], lv[bad[0]], lo[bad[0]], hi[bad[0]])
        if l:  # the maximum over four entries of the level below, as the device holds that level
            prev = levels[l - 1]
            pooled = np.concatenate([prev, np.zeros(-len(prev) % 4, np.int64)]).reshape(-1, 4).max(axis=1)
            want = np.zeros(len(lv), np.int64)
            n = min(len(lv), len(pooled))
            want[:n] = pooled[:n]
            _eq(lv, want, "%s: level %d pooled from level %d" % (what, l, l - 1))
    assert rmax_list == levels[0].max(), (what, rmax_list, levels[0].max())
    return int(near.sum()), len(docs)


def check_list_max(world, t, rmax_list, what):
    """rmax_list of a list that keeps only that (a range directory, no bitmap)"""
    tt = world.model(t, "t")
    byte, near = PM.rmax_byte(tt), PM.rmax_near_integer(tt).astype(np.int64)
    assert rmax_list / 255.0 >= tt.max(), (what, rmax_list)
    assert (byte - near).max() <= rmax_list <= np.minimum(255, byte + near).max(), (what, rmax_list, byte.max())


def check_term(world, dev, t, h, what, field=0, idx_base=0, pos_base=0):
    """Every per-term table of list t (handle h) against the models.  -> its info"""
    c = world.case
    pl, seg = c.lists[t], c.seg
    docs, tfs = PM.arrays(pl)
    df = len(pl)
    info = dev.term_table_info(h)
    ti = seg.terms[t]
    # ---- the facts
    rec = world.model(t, "rec")
    assert (info["doc_freq"], info["n_blocks"], info["n_full"], info["n_tail"]) == (df, (df + 127) // 128, df // 128, df % 128), (what, info)
    shift, coarse = world.model(t, "coarse")
    assert info["coarse_shift"] == shift, (what, info)
    skip_bytes = 0
    if df >= 128:
        skip_len, at = PM._vint_stop_last(seg.postings_bytes(t), 0)
        skip_bytes = at + skip_len
    assert info["payload_base"] == idx_base + 8 + ti.postings_start + skip_bytes, (what, info)
    assert info["has_freq"] & 1 == (1 if c.has_freq else 0) and info["has_freq"] >> 29 == 0 and not info["has_freq"] & 0xFE, (what, info)
    assert (info["has_freq"] >> 26) & 7 == field and info["field"] == field and not info["has_freq"] >> 25 & 1, (what, info)
    n_pos = int(tfs.sum()) if c.with_positions else 0
    assert (info["n_positions"], info["n_pos_blocks"], info["n_pos_tail"]) == (n_pos, n_pos // 128, n_pos % 128), (what, info)
    # ---- the unrolled skip list
    _eq(dev.term_table(h, "rec"), rec, what + " rec")
    _eq(dev.term_table(h, "coarse"), coarse, what + " coarse")
    tail_docs, tail_tfs = PM.tails(pl, c.has_freq)
    _eq(dev.term_table(h, "tail_docs"), tail_docs, what + " tail_docs")
    _eq(dev.term_table(h, "tail_tfs"), tail_tfs, what + " tail_tfs")
    if c.with_positions:  # positions/reader.rs: VInt n_blocks, a width byte per block, the bit-packed blocks, the vint tail
        pb = seg.pos[ti.positions_start: ti.positions_end]
        nb, at = PM._vint_stop_last(pb, 0)
        widths = pb[at: at + nb].astype(np.int64)
        offs = pos_base + ti.positions_start + at + nb + np.concatenate([[0], np.cumsum(16 * widths)])[:nb]
        got = dev.term_table(h, "pos_blk")
        _eq(got & np.uint64((1 << 56) - 1), offs, what + " pos_blk offsets")
        _eq(got >> np.uint64(56), widths, what + " pos_blk widths")
        deltas = np.concatenate([np.minimum(np.arange(tf), 1) for tf in tfs.tolist()])  # (positions 0 .. tf - 1)
        _eq(dev.term_table(h, "pos_tail"), deltas[128 * nb:], what + " pos_tail")
    # ---- the side tables
    is_dense = c.is_dense(t)
    S = 0 if is_dense else PM.rdir_shift(c.max_doc, df)
    assert info["rdir_shift"] == S, (what, info, S)
    for name in ("dense", "tf8", "rmax") + (("bits", "pos_dir") if c.with_positions else ()):
        if not is_dense and info["probe_slot"] == NONE:
            assert dev.term_table(h, name).size == 0, (what, name)
    if is_dense:
        _eq(dev.term_table(h, "dense"), world.model(t, "dense"), what + " dense")
        _eq(dev.term_table(h, "tf8"), PM.tf8(pl) if c.has_freq else np.ones(df), what + " tf8")
        if c.with_positions:
            _eq(dev.term_table(h, "bits"), PM.bits(c.max_doc, pl), what + " bits")
            _eq(dev.term_table(h, "pos_dir"), PM.pos_dir(pl), what + " pos_dir")
        else:
            assert dev.term_table(h, "bits").size == 0 and dev.term_table(h, "pos_dir").size == 0
        assert dev.term_table(h, "rdir").size == 0
        if field == 0:
            info["near"] = check_rmax(world, t, dev.term_table(h, "rmax"), info["rmax_list"], what + " rmax")
        else:
            assert dev.term_table(h, "rmax").size == 0 and info["rmax_list"] == 255, (what, info)
    elif S:
        directory, entries = PM.rdir(c.max_doc, pl, S)
        got = dev.term_table(h, "rdir")
        n_dir = PM.rdir_dir_words(c.max_doc, S)
        assert len(got) == n_dir + df, (what, len(got))
        _eq(got[:len(directory)], directory, what + " rdir directory (shift %d)" % S)
        _eq(got[n_dir:], entries, what + " rdir entries")
        if field == 0 and info["probe_slot"] == NONE:
            check_list_max(world, t, info["rmax_list"], what + " rmax_list")
        elif field:
            assert info["rmax_list"] == 255, (what, info)
    else:
        assert dev.term_table(h, "rdir").size == 0
        if info["probe_slot"] == NONE:
            assert info["rmax_list"] == 255, (what, info)
    return info


def check_matrices(world, dev, infos, what, fieldnorm_ids="case"):
    """docmat and doccls against the models built from {t: info} of the lists that are prepared; every other bit zero."""
    c = world.case
    columns, cls_columns, sigs = {}, {}, []
    for t, info in infos.items():
        slot, bit, cls = _slot_bit(info)
        assert -1 <= slot < PM.MAT_SLOTS and -1 <= bit < PM.SIG_BITS and not (slot >= 0 and bit >= 0), (what, t, info)
        if slot >= 0:
            assert slot not in columns, (what, slot)
            columns[slot] = c.lists[t]
            assert cls == (slot < PM.CLS_SLOTS), (what, t, info)
            if cls:
                cls_columns[slot] = c.lists[t] if c.has_freq else [(d, 1) for d, _ in c.lists[t]]
        else:
            assert not cls
        if bit >= 0:
            sigs.append((bit, c.lists[t]))
    fn = c.fieldnorm_ids if isinstance(fieldnorm_ids, str) else fieldnorm_ids
    got = dev.term_table(0, "docmat")
    want = PM.docmat(c.max_doc, fn, world.const_id, columns, sigs)
    if not np.array_equal(got, want):
        at = np.nonzero(got != want)[0]
        raise AssertionError("%s docmat: %d docs differ, first %d: got %#x, want %#x" % (what, len(at), at[0], got[at[0]], want[at[0]]))
    got = dev.term_table(0, "doccls")
    if columns:
        want = PM.doccls(c.max_doc, cls_columns)
        if not np.array_equal(got, want):
            at = np.nonzero(got != want)[0]
            raise AssertionError("%s doccls: %d docs differ, first %d: got %#x, want %#x" % (what, len(at), at[0], got[at[0]], want[at[0]]))
    else:
        assert got.size == 0
    return columns, sigs


def check_segment_words(world, dev):
    c = world.case
    got = dev.term_table(0, "local_cache")
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), world.cache.view(np.uint32))
    want_min = int(c.fieldnorm_ids.min()) if c.fieldnorm_ids is not None else 1
    assert dev.term_table(0, "min_fieldnorm_id").tolist() == [want_min]


def check_columns_in_order(world, infos):
    """The columns are reserved for the segment's TQD_MAT_SLOTS longest lists (DeviceIndex.add_segment names them with
    tq_segment_reserve_columns: by doc freq, then by postings offset); those of them that are dense take the slots in the
    order they are prepared (term order here); every other list of a segment of 4 096 docs or more has a signature bit."""
    c = world.case
    by_df = sorted(range(len(c.lists)), key=lambda t: (-len(c.lists[t]), c.seg.terms[t].postings_start))
    reserved = set(by_df[:PM.MAT_SLOTS])
    rank = 0
    for t in sorted(infos):
        slot, bit, _ = _slot_bit(infos[t])
        if c.is_dense(t) and t in reserved:
            assert slot == rank, (t, rank, slot)
            rank += 1
        else:
            assert slot == -1, (t, slot)
    for t, info in infos.items():
        slot, bit, _ = _slot_bit(info)
        assert (bit >= 0) == (slot < 0), (t, info)


# ---------------------------------------------------------------- the builders against the models
@pytest.mark.parametrize("path,use_dpp", PATHS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_every_table_of_every_list(ta, worlds, name, path, use_dpp):
    world = worlds(name)
    c = world.case
    dev = _open(ta, c, use_dpp)
    try:
        ids = list(range(len(c.lists)))
        hs = _prepare(ta, dev, c.seg, ids, path)
        assert sorted(hs) == ids
        check_segment_words(world, dev)
        infos = {t: check_term(world, dev, t, hs[t], "%s %s list %d (%s)" % (name, path, t, c.notes[t])) for t in ids}
        if path != "batch":  # (a batch prepares its dense lists first: the same columns, other handles)
            assert hs == ids
        check_columns_in_order(world, infos)
        columns, sigs = check_matrices(world, dev, infos, "%s %s" % (name, path))
        n_dense = sum(c.is_dense(t) for t in ids)
        assert len(columns) == min(PM.MAT_SLOTS, n_dense)
        if name == "A":  # columns run out, classes run out before them, every signature bit is shared
            assert n_dense > PM.MAT_SLOTS and max(columns) >= PM.CLS_SLOTS
            assert all(sum(1 for b, _ in sigs if b == bit) >= 2 for bit in set(b for b, _ in sigs)) and len(sigs) > PM.MAT_SLOTS + PM.SIG_BITS
        near = [i["near"] for i in infos.values() if "near" in i]
        assert near and sum(n for n, _ in near) * 100 < sum(n for _, n in near), near
        assert sum(1 for t in ids if infos[t]["rdir_shift"]) >= 4
    finally:
        dev.close()


def test_basic_records(ta, worlds):
    """has_freq 0: every tf reads as 1 in the tails, the tf bytes, the classes and the directory entries"""
    world = worlds("basic")
    c = world.case
    for path in ("host", "device", "batch"):
        dev = _open(ta, c)
        try:
            ids = list(range(len(c.lists)))
            hs = _prepare(ta, dev, c.seg, ids, path)
            infos = {t: check_term(world, dev, t, hs[t], "basic %s list %d" % (path, t)) for t in ids}
            check_matrices(world, dev, infos, "basic " + path)
        finally:
            dev.close()


def test_rank_directory_across_scan_tiles_and_the_carry(ta, worlds):
    """Segment C: 258 scan tiles of 2 048 bitmap words — the one workgroup that scans the tile sums takes a second chunk
    of 256 and carries the first chunk's total into it; postings on both sides, and in the last word."""
    world = worlds("C")
    c = world.case
    dev = _open(ta, c)
    try:
        ids = list(range(len(c.lists)))
        hs = _prepare(ta, dev, c.seg, ids, "host")
        check_segment_words(world, dev)
        infos = {t: check_term(world, dev, t, hs[t], "C list %d" % t) for t in ids}
        for t in ids:  # the rank words beyond the first chunk of tiles carry what came before
            d = dev.term_table(hs[t], "dense")
            before = int((PM.arrays(c.lists[t])[0] < 256 * 2048 * 32).sum())
            assert 0 < before < len(c.lists[t]) and d[256 * 2048, 1] == before and d[-1, 1] == len(c.lists[t])
        check_matrices(world, dev, infos, "C")
    finally:
        dev.close()


# ---------------------------------------------------------------- tables built on first use
def _tree(ta, spec):
    """[(occur, term | [(occur, term | ("ph", [terms]))] , msm)] -> a query tuple of DeviceIndex.search"""
    terms, occ, cof, nested, atom, offs = [], [], [], [], [], []
    for ci, cl in enumerate(spec):
        members = cl[1] if isinstance(cl[1], list) else [(M, cl[1])]
        for mi, (inner, member) in enumerate(members):
            phrase = isinstance(member, tuple)
            for o, t in enumerate(member[1] if phrase else [member]):
                terms.append(t), occ.append(cl[0]), cof.append(ci), atom.append(mi)
                nested.append(inner | (0x10 if phrase else 0)), offs.append(o if phrase else 0)
    return (ta.MODE_BOOL, terms, occ, cof, 0, {"nested_occurs": nested, "atom_of": atom, "phrase_offsets": offs})


def test_probe_pool_tables_of_lists_below_dense_ratio(ta, worlds):
    """A nested boolean query reaches every list through a bitmap: lists below "dense_ratio" get bitmap + rank directory
    and tf bytes in a slot of the probe pool the first time one names them, a position directory the first time a phrase
    inside one does — the same tables as a list's own, by the same models; their range maxima live in the slot too."""
    world = worlds("A")
    c = world.case
    dev = _open(ta, c)
    try:
        ids = list(range(len(c.lists)))
        hs = _prepare(ta, dev, c.seg, ids, "host")
        a, b, r, d = c.by_note("length 255")[0], c.by_note("length 257")[0], c.by_note("gaps rdir")[0], c.by_note("runs dense")[0]
        assert not c.is_dense(a) and not c.is_dense(b) and not c.is_dense(r) and c.is_dense(d)
        dev.search([_tree(ta, [(M, [(M, ("ph", [a, b]))], 0), (S_, d)]), _tree(ta, [(M, d), (M, [(M, r), (S_, a)], 0)])], 5)
        assert "tree" in dev.last_batch_stats()["kernels"]
        infos = {}
        for t in (a, b, r):
            what = "A probe list %d (%s)" % (t, c.notes[t])
            infos[t] = info = check_term(world, dev, t, hs[t], what)  # (its own tables are as before)
            assert info["probe_slot"] != NONE, (what, info)
            _eq(dev.term_table(hs[t], "probe_dense"), world.model(t, "dense"), what + " probe dense")
            _eq(dev.term_table(hs[t], "probe_tf8"), PM.tf8(c.lists[t]), what + " probe tf8")
            if t != r:
                _eq(dev.term_table(hs[t], "probe_pos_dir"), PM.pos_dir(c.lists[t]), what + " probe pos_dir")
            check_rmax(world, t, dev.term_table(hs[t], "rmax"), info["rmax_list"], what + " rmax (in the slot)")
            assert dev.term_table(hs[t], "dense").size == 0  # (the other kernels keep seeing the list as sparse)
        assert len({infos[t]["probe_slot"] for t in infos}) == 3
        # ... and nothing of it reached the matrices
        all_infos = {t: dev.term_table_info(hs[t]) for t in ids}
        check_matrices(world, dev, all_infos, "A after probe tables")
    finally:
        dev.close()


def test_leader_norms_and_plain_arrays(ta, worlds):
    """lnorm: built the first time a list leads queries of a shared-intersection launch; flat: the first time an
    unpruned doc-major union names a list without a bitmap."""
    world = worlds("A")
    c = world.case
    dev = _open(ta, c, ashare_min_batch=0, xunion_ratio=1 << 30, xunion_min_queries=1)
    try:
        ids = list(range(len(c.lists)))
        hs = _prepare(ta, dev, c.seg, ids, "host")
        big = c.by_note("length %d" % (65 * 128 + 77))[0]
        leaders = [c.by_note("length %d" % df)[0] for df in (1, 127, 128, 129, 257)] + c.by_note("rdir")
        dev.set_option("exhaustive", 0)
        dev.search([(O.MODE_AND, [t, big]) for t in leaders], 10)
        assert dev.last_batch_stats()["kernel_mask"] & ta.binding.KERNEL_ASHARE
        built = 0
        for t in ids:
            got = dev.term_table(hs[t], "lnorm")
            if got.size:
                built += 1
                _eq(got, PM.lnorm(c.lists[t], c.fieldnorm_ids), "A lnorm list %d (%s)" % (t, c.notes[t]))
        assert built >= len(leaders) and all(dev.term_table(hs[t], "lnorm").size for t in leaders)
        sparse = [t for t in ids if not c.is_dense(t)]
        dev.set_option("exhaustive", 1)
        dev.search([(O.MODE_OR, [sparse[i], sparse[i + 1], sparse[i + 2]]) for i in range(0, len(sparse) - 2, 3)], 10)
        assert "xunion" in dev.last_batch_stats()["kernels"], dev.last_batch_stats()
        built = 0
        for t in sparse:
            got = dev.term_table(hs[t], "flat")
            if got.size:
                built += 1
                docs, off, tf8 = PM.flat(c.lists[t])
                assert got.size == off + len(docs)
                _eq(got[:4 * len(docs)].view(np.uint32), docs, "A flat docs list %d" % t)
                _eq(got[off:], tf8, "A flat tf bytes list %d" % t)
        assert built >= 10, built
    finally:
        dev.close()


# ---------------------------------------------------------------- life cycle
@pytest.fixture(scope="module")
def life():
    """The segment of test_device_side_prepare_reports_corrupt_lists (tests/test_gpu_round2.py) with good lists behind its
    one list, and the copy with the same four zeroed bytes: last_doc of skip entry 5 := 0."""
    from tests.helpers import random_postings

    rng = np.random.default_rng(5)
    first = random_postings(rng, 50_000, 3000, max_tf=5)
    fieldnorms = rng.integers(1, 50, size=50_000).tolist()
    rng2 = np.random.default_rng(55)
    lists = [first, random_postings(rng2, 50_000, 2500, max_tf=5), random_postings(rng2, 50_000, 1000, max_tf=3)]
    lists += [random_postings(rng2, 50_000, int(rng2.integers(40, 200)), max_tf=4) for _ in range(40)]
    seg = O.build_segment(50_000, lists, fieldnorms)
    only = O.build_segment(50_000, [first], fieldnorms)
    n0 = only.terms[0].postings_end
    assert np.array_equal(seg.idx[8:8 + n0], only.idx[8:8 + n0])  # (the suite's corrupt input, byte for byte)
    bad = O.Segment(seg.max_doc, seg.record_option, seg.idx[: seg.idx_len].copy(), np.zeros(0, np.uint8), seg.fieldnorm,
                    seg.terms, seg.total_num_tokens)
    bad.idx[8 + 3 + 8 * 5:8 + 3 + 8 * 5 + 4] = 0
    case = PC.Case.wrap("life", bad, lists, seg.fieldnorm, 128, with_positions=False)
    return World(case)


def test_nothing_of_a_rejected_list_a_released_set_or_an_evicted_slot_stays_in_the_matrices(ta, life):
    c = life.case
    for walk in (0, 1):
        dev = ta.DeviceIndex([c.seg])
        try:
            dev.set_option("device_prepare", walk)
            dev.set_option("dense_budget_x", 64)
            dev.set_option("probe_budget_x", 1)  # (the pool's floor: a query's worth of slots, 16)
            dev.set_option("rdir_budget_x", 0)
            rc, _ = _prepare_one_rc(ta, dev, c.seg, 0)
            assert rc == TQ_ERR_FORMAT, (rc, ta.binding.lib().tq_last_error())
            good = list(range(1, len(c.lists)))
            hs = {t: _prepare_one(ta, dev, c.seg, t) for t in good}
            infos = {t: check_term(life, dev, t, hs[t], "life walk %d list %d" % (walk, t)) for t in good}
            assert _slot_bit(infos[1])[0] == 0 and _slot_bit(infos[2])[0] == 1  # (the rejected list took no column)
            check_matrices(life, dev, infos, "after a rejected list (walk %d)" % walk)
            rc, _ = _prepare_one_rc(ta, dev, c.seg, 0)
            assert rc == TQ_ERR_FORMAT
            check_matrices(life, dev, infos, "after the rejected list again (walk %d)" % walk)
            # a term set over column, signature and sparse lists, released
            st = dev.term_set_prepare([1, 2, 5, 9])
            assert dev.term_table(st, "dense").size and dev.term_table(st, "rec").size == 0
            dev.term_set_release(st)
            with pytest.raises(ta.TantivyAmdError):
                dev.term_table(st, "dense")
            check_matrices(life, dev, {t: dev.term_table_info(hs[t]) for t in good}, "after a released term set (walk %d)" % walk)
            # nested queries over more sparse lists than the pool has slots: the oldest owners are evicted
            sparse = good[2:]
            for i in range(0, len(sparse) - 1, 2):
                dev.search([_tree(ta, [(M, 1), (N, [(M, sparse[i]), (M, sparse[i + 1])], 0)])], 5)  # +a -(+b +c)
                assert "tree" in dev.last_batch_stats()["kernels"]
            assert dev.segment_stats(0)["probe_evictions"] > 0
            slots = {t: dev.term_table_info(hs[t])["probe_slot"] for t in sparse}
            held = [t for t in sparse if slots[t] != NONE]
            assert 0 < len(held) < len(sparse) and len({slots[t] for t in held}) == len(held)
            for t in sparse:
                got = dev.term_table(hs[t], "probe_dense")
                if slots[t] == NONE:  # evicted: the list is as it was prepared
                    assert got.size == 0 and dev.term_table(hs[t], "rmax").size == 0
                else:  # a slot taken over holds nothing of its former owner
                    _eq(got, life.model(t, "dense"), "life probe dense of list %d in a reused slot" % t)
                    _eq(dev.term_table(hs[t], "probe_tf8"), PM.tf8(c.lists[t]), "life probe tf8 of list %d" % t)
                    check_rmax(life, t, dev.term_table(hs[t], "rmax"), dev.term_table_info(hs[t])["rmax_list"], "life rmax of list %d" % t)
            check_matrices(life, dev, {t: dev.term_table_info(hs[t]) for t in good}, "after evictions (walk %d)" % walk)
        finally:
            dev.close()


# ---------------------------------------------------------------- a multi-field segment
def _upload_fields_raw(ta, dev, fx):
    """tq_segment_upload_fields through the raw C ABI on `dev`'s context: no columns are reserved, so a dense list of any
    field takes the next free one.  -> (the segment, what has to outlive it); dev's table readers then read THIS segment."""
    B = ta.binding
    ff, keep = (B.TqFieldFiles * len(fx.fields))(), []
    for f, seg in enumerate(fx.fields):
        idx = np.ascontiguousarray(seg.idx[: seg.idx_len], dtype=np.uint8)
        pos = np.ascontiguousarray(seg.pos[: seg.pos_len], dtype=np.uint8)
        fn = None if seg.fieldnorm is None else np.ascontiguousarray(seg.fieldnorm, dtype=np.uint8)
        keep += [idx, pos, fn]
        ff[f] = B.TqFieldFiles(idx.ctypes.data, idx.size, pos.ctypes.data if pos.size else None, pos.size,
                               fn.ctypes.data if fn is not None else None, fn.size if fn is not None else 0)
    raw = C.c_void_p()
    rc = B.lib().tq_segment_upload_fields(dev.ctx, 0, fx.max_doc, len(fx.fields), ff, fx.fields[0].record_option, C.byref(raw))
    assert rc == 0, B.lib().tq_last_error()
    dev.segment_raw = lambda segment_ord=0: raw
    return raw, keep


@pytest.mark.parametrize("upload", ["mirror", "raw"])
def test_a_list_of_a_non_primary_field(ta, upload):
    """tests/fields_model.py's two-field fixture: a list of field 1 has no range maxima (rmax_list 255), its bitmap,
    rank directory and range directory are the models' under the shifted offsets, and its membership bit lives in the one
    doc matrix next to field 0's: a signature bit through DeviceIndex.add_segment_fields (which reserves the columns for
    field 0's longest lists), a column through the raw upload (nothing reserved)."""
    from tests import fields_model as FM

    fx = FM.fixture_y()
    f0, f1 = fx.fields
    lib = ta.binding.lib()
    dev = ta.DeviceIndex()
    raw = None
    try:
        if upload == "mirror":
            assert dev.add_segment_fields(fx.fields) == fx.bases[:-1]
        else:
            raw, keep = _upload_fields_raw(ta, dev, fx)
        dev.set_option("dense_budget_x", 64, 0)

        def handle(f, t):
            if upload == "mirror":
                return dev.term_handle(fx.gid(f, t))
            ti, h = fx.fields[f].terms[t], C.c_uint32(NONE)
            rc = lib.tq_term_prepare_field(raw, f, ti.postings_start, ti.postings_end - ti.postings_start, ti.positions_start,
                                           ti.positions_end - ti.positions_start, ti.doc_freq, C.byref(h))
            assert rc == 0, lib.tq_last_error()
            return int(h.value)

        lists1 = [list(zip(*(a.tolist() for a in O.decode_postings(f1, t)))) for t in range(len(f1.terms))]
        case = PC.Case.wrap("Y1", f1, lists1, fx.fn_ids(1), 128, with_positions=True)
        world = World(case)
        bases = set()  # where field 1's .idx sub-file lies: one offset for all of its lists, behind field 0's
        hs = {t: handle(1, t) for t in range(len(lists1))}
        h0 = handle(0, 0)
        infos = {}
        for t, h in hs.items():
            info = dev.term_table_info(h)
            assert info["field"] == 1 and info["rmax_list"] == 255 and dev.term_table(h, "rmax").size == 0, info
            pl = lists1[t]
            if case.is_dense(t):
                _eq(dev.term_table(h, "dense"), PM.dense(fx.max_doc, pl), "field 1 dense list %d" % t)
                _eq(dev.term_table(h, "tf8"), PM.tf8(pl), "field 1 tf8 list %d" % t)
                _eq(dev.term_table(h, "pos_dir"), PM.pos_dir(pl), "field 1 pos_dir list %d" % t)
                _eq(dev.term_table(h, "bits"), PM.bits(fx.max_doc, pl), "field 1 bits list %d" % t)
            S = 0 if case.is_dense(t) else PM.rdir_shift(fx.max_doc, len(pl))
            assert info["rdir_shift"] == S
            if S:
                directory, entries = PM.rdir(fx.max_doc, pl, S)
                got = dev.term_table(h, "rdir")
                _eq(got[:len(directory)], directory, "field 1 rdir directory list %d" % t)
                _eq(got[PM.rdir_dir_words(fx.max_doc, S):], entries, "field 1 rdir entries list %d" % t)
            _eq(dev.term_table(h, "rec"), PM.rec(pl, f1.postings_bytes(t), f1.record_option, True), "field 1 rec list %d" % t)
            skip = sum(PM._vint_stop_last(f1.postings_bytes(t), 0)) if len(pl) >= 128 else 0
            bases.add(info["payload_base"] - (8 + f1.terms[t].postings_start + skip))
            infos[t] = info
        assert len(bases) == 1 and min(bases) >= f0.idx_len, bases
        dense1 = [t for t in infos if case.is_dense(t)]
        assert len(dense1) >= 3 and sum(1 for t in infos if infos[t]["rdir_shift"]) >= 1
        for t in dense1:
            slot, bit, _ = _slot_bit(infos[t])
            assert (slot >= 0) == (upload == "raw") and (bit >= 0) == (upload == "mirror"), (t, infos[t])
        # the one doc matrix: field 0's fieldnorm ids in the low byte, field 1's bits next to field 0's
        info0 = dev.term_table_info(h0)
        lists0 = list(zip(*(a.tolist() for a in O.decode_postings(f0, 0))))
        case.lists = lists1 + [lists0]
        infos[len(lists1)] = info0
        check_matrices(world, dev, infos, "two fields (%s)" % upload, fieldnorm_ids=np.asarray(fx.fn_ids(0), np.int64))
    finally:
        if raw is not None:
            lib.tq_segment_free(raw)
        dev.close()
