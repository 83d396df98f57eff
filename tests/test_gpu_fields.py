"""GPU parity of multi-field segments (tq_segment_upload_fields, tq_term_prepare_field / _batch_fields, tq_term_field:
tantivy_amd/csrc/tq_fields.cpp; tree_fields_kernel, docset_score_fields_kernel) through tq_search_batch, tq_search_one,
tq_count_batch, tq_docset_batch, tq_docset_scored_batch and the host mirror's DeviceIndex.add_segment_fields.

Expectations never come from the device: tests/fields_model.py (oracle decode + oracle BM25 per field, the literal model of
tests/all_model.py over lists keyed by global term id, tests/phrase_model.py for phrases).  tests/test_fields_cpu.py shows
that the same model under field 0's norms for every term differs on every scored case below.  Comparison rule
(tests/test_gpu_docset_scored.py): docs and counts exact; scores bit for bit with at most two scoring lists, within 1e-5
relative otherwise — and for every query with a phrase, whose expectation is phrase_model's float64 definition (f32
evaluation of w * c / (c + norm) is three roundings, 2^-24 relative each: far inside 1e-5); top-k rows exact (score, doc)
sequences with at most two scoring lists."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import all_model as AM
from tests import fields_model as FM
from tests import phrase_model as PM
from tests.test_gpu_all import ABSENT_ID, Lists, T, check_cases
from tests.test_gpu_round3 import _alive_bytes
from tests.tree_shapes import to_device

pytestmark = pytest.mark.gpu

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
ERR_INVALID, ERR_UNSUPPORTED = 1, 4
KERNEL_TREE = 0x1000
TERMINATED = 0x7FFFFFFF


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


def _err(ta):
    return ta.binding.lib().tq_last_error()


def _open(ta, fx):
    dev = ta.DeviceIndex()
    assert dev.add_segment_fields(fx.fields) == fx.bases[:-1]
    return dev


def _deleted(fx):
    rng = np.random.default_rng(7)
    dele = set(int(d) for d in rng.choice(fx.max_doc, size=fx.max_doc // 5, replace=False))
    dele.update(d for d in (0, 31, 65536, fx.max_doc - 1) if d < fx.max_doc)
    return sorted(dele)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. a query of field-0 terms alone runs exactly as on a single-field upload of field 0
def _primary_queries(fx):
    seg0 = fx.fields[0]
    by_df = sorted(range(len(seg0.terms)), key=lambda t: seg0.terms[t].doc_freq)
    hi = by_df[-5:]
    phrase = (O.MODE_PHRASE, [0, 1], [0, 1]) if fx.name == "Y" else (O.MODE_PHRASE, [hi[-1], hi[-2]], [0, 2])
    flat = [(O.MODE_AND, hi[-2:], None), (O.MODE_AND, hi[-3:], None), (O.MODE_OR, hi, None), phrase,
            (O.MODE_BOOL, [hi[-1], hi[-2], hi[-3]], None, [M, S, N], None, 0), (O.MODE_AND, [by_df[0], hi[-1]], None)]
    nested = [(M, hi[-1]), (M, [(M, hi[-2]), (S, hi[-3]), (N, hi[-4])], 0)]  # +a +(+b c -d)
    return flat, nested


@pytest.mark.parametrize("name", ["X", "Y"])
def test_primary_only_parity(ta, name):
    fx = FM.FIXTURES[name]()
    seg0 = fx.fields[0]
    L0 = Lists(seg0)
    caches = fx.caches()
    assert np.array_equal(_bits(caches[0]), _bits(L0.cache))
    flat, nested = _primary_queries(fx)
    for q in flat:
        for t in q[1]:
            L0.need(t)

    def weights_of(q):
        if q[0] == O.MODE_PHRASE:
            return [float(O.bm25_for_terms([seg0.terms[t].doc_freq for t in q[1]], seg0.max_doc, L0.avg).weight)]
        return [L0.weights[t] for t in q[1]]

    ws = [weights_of(q) for q in flat]
    tree_q = to_device(ta, nested, 0)
    for t in tree_q[1]:
        L0.need(t)
    tree_w = [[L0.weights[t] for t in tree_q[1]]]
    docq = [(q[0], q[1], q[2]) if q[0] == O.MODE_PHRASE else ((q[0], q[1], q[3], q[4], q[5]) if q[0] == O.MODE_BOOL else (q[0], q[1]))
            for q in flat] + [tree_q]
    out = {}
    for which in ("single", "multi"):
        dev = ta.DeviceIndex([seg0]) if which == "single" else _open(ta, fx)
        cache = L0.cache if which == "single" else caches
        try:
            if which == "multi":  # the segment holds prepared terms of other fields: the pre-pass looks at every query
                for f in range(1, len(fx.fields)):
                    assert dev.term_field(dev.term_handle(fx.gid(f, 0))) == f
                assert dev.fields_stats()["n_field_terms"] == len(fx.fields) - 1
            dev.set_option("record_query_kernels", 1)
            dev.set_option("docset_trees", 1)
            dev.set_option("docset_score_trees", 1)
            got = []
            for ex in (0, 1):
                sc, dc, ct = dev.raw_search(flat, ws, cache, 10, opts=(ex, 0))
                got += [_bits(sc).copy(), dc.copy(), ct.copy(), dev.last_batch_query_kernels(len(flat)).copy()]
                sc, dc, ct = dev.raw_search_trees([tree_q], tree_w, cache, 10, opts=(ex, 0))
                got += [_bits(sc).copy(), dc.copy(), ct.copy(), dev.last_batch_query_kernels(1).copy()]
            for q, w in zip(flat, ws):
                one = (q[0], q[1], q[2]) if q[0] == O.MODE_PHRASE else ((q[0], q[1], q[3], q[4], q[5]) if q[0] == O.MODE_BOOL else (q[0], q[1]))
                s1, d1, c1 = dev.raw_search_one(one, w, cache, 10)
                got += [_bits(s1).copy(), d1.copy(), np.array([c1])]
            got.append(dev.raw_count(flat, ws, cache).copy())
            rc, docs, starts = dev.raw_docset(docq, 1 << 18)
            assert rc == 0, _err(ta)
            got += [docs[: int(starts[-1])].copy(), starts.copy()]
            rc, sdocs, scores, sstarts = dev.raw_docset_scored(docq, 1 << 18, weights=ws + tree_w, cache=cache)
            assert rc == 0, _err(ta)
            got += [sdocs[: int(sstarts[-1])].copy(), _bits(scores[: int(sstarts[-1])]).copy(), sstarts.copy()]
            out[which] = got
        finally:
            dev.close()
    assert len(out["single"]) == len(out["multi"])
    for i, (a, b) in enumerate(zip(out["single"], out["multi"])):
        assert np.array_equal(a, b), (i, a[:8], b[:8])
    assert int(out["single"][-2].size) > 0 and KERNEL_TREE not in out["single"][3].tolist()[:3]


# ---- 2. single-term and flat queries of each non-primary field and of mixed fields
@pytest.mark.parametrize("with_deletes", [False, True])
@pytest.mark.parametrize("name", ["X", "Y"])
def test_flat_queries_of_any_field_mix(ta, name, with_deletes):
    fx = FM.FIXTURES[name]()
    L = FM.FieldLists(fx)
    cases = FM.flat_cases(fx)
    alive = None
    dev = _open(ta, fx)
    try:
        if with_deletes:
            dele = _deleted(fx)
            alive = np.ones(fx.max_doc, bool)
            alive[dele] = False
            dev.set_alive_bitset(_alive_bytes(fx.max_doc, dele))
        want, rows = check_cases(ta, dev, L, cases, alive=alive, ks=(1, 10, 100))
        assert all(w[0].size > 0 for w in want)
        for k in (1, 10, 100):  # nothing is pruned: "exhaustive" 0 and 1 give the same rows — EVERY row, bit for bit
            for x, y in zip(rows[(k, 0)], rows[(k, 1)]):
                assert np.array_equal(_bits(x), _bits(y)), k
        # nothing is pruned: the doc-set size after either mode, TQ_KERNEL_TREE whatever the query's mode
        from tests.test_gpu_all import _entries, _weights_of

        srch, ws = [], []
        for c, m in cases:
            t, o, cof, whats = _entries(c)
            srch.append((ta.MODE_BOOL, t, None, o, cof, m))
            ws.append(_weights_of(whats, L))
        # the TQ_MODE_OR / TQ_MODE_AND spellings of the flat all-Should / all-Must cases ride along
        spell = [(O.MODE_OR, [cases[0][0][0][1][1]], None),
                 (O.MODE_AND, [w[1] for _, w in cases[3][0]], None), (O.MODE_OR, [w[1] for _, w in cases[4][0]], None)]
        spell_w = [[L.weights[t] for t in q[1]] for q in spell]
        spell_want = [want[0], want[3], want[4]]
        dev.set_option("record_query_kernels", 1)
        for ex in (0, 1):
            sc, dc, ct = dev.raw_search(srch + spell, ws + spell_w, L.cache, 10, opts=(ex, 0))
            n = len(srch) + len(spell)
            assert dev.last_batch_match_counts(n).tolist() == [w[0].size for w in want + spell_want], ex
            assert dev.last_batch_query_kernels(n).tolist() == [KERNEL_TREE] * n, ex
            for i, (wd, wsc) in enumerate(spell_want):  # (each has at most two scoring lists, or is compared at 1e-5)
                j = len(srch) + i
                c = int(ct[j])
                es, ed = AM.top_k(wd, wsc, 10)
                assert c == min(10, wd.size)
                if len(spell[i][1]) <= 2:
                    assert np.array_equal(dc[j, :c], ed) and np.array_equal(_bits(sc[j, :c]), _bits(es)), spell[i]
                else:
                    assert np.allclose(np.sort(sc[j, :c])[::-1], es, rtol=1e-5, atol=0), spell[i]
        # tq_search_one gives the batch's row
        sc, dc, ct = rows[(10, 0)]
        for i, (c, m) in enumerate(cases[:6]):
            t, o, cof, whats = _entries(c)
            s1, d1, c1 = dev.raw_search_one((ta.MODE_BOOL, t, o, cof, m), _weights_of(whats, L), L.cache, 10)
            assert c1 == int(ct[i]) and np.array_equal(d1[:c1], dc[i, :c1]) and np.array_equal(_bits(s1[:c1]), _bits(sc[i, :c1])), c
    finally:
        dev.close()


# ---- 3. nested shapes, phrase atoms and standalone phrases with a field != 0
def _check_topk(sc, dc, ct, want, k, exact, what):
    wd, ws = want
    c = int(ct)
    assert c == min(k, wd.size), (what, k, c, wd.size)
    assert np.all(sc[c:] == 0.0) and np.all(dc[c:] == TERMINATED), what
    if exact:
        es, ed = AM.top_k(wd, ws, k)
        assert np.array_equal(dc[:c], ed) and np.array_equal(_bits(sc[:c]), _bits(es)), (what, k)
        return
    pos = np.searchsorted(wd, dc[:c])
    assert np.all(pos < max(1, wd.size)) and np.array_equal(wd[np.minimum(pos, max(0, wd.size - 1))], dc[:c]), what
    assert np.allclose(sc[:c], ws[pos], rtol=1e-5, atol=0), (what, sc[:4], ws[pos][:4])
    if c:  # no better doc is missing
        last = float(sc[c - 1])
        missing = np.setdiff1d(np.nonzero(ws > last + abs(last) * 1e-5)[0], pos)
        assert missing.size == 0, (what, k, wd[missing][:4])


@pytest.mark.parametrize("with_deletes", [False, True])
@pytest.mark.parametrize("name", ["X", "Y"])
def test_nested_shapes_and_phrase_atoms(ta, name, with_deletes):
    fx = FM.FIXTURES[name]()
    L = FM.FieldLists(fx)
    cases = FM.tree_cases(fx)
    alive = None
    dev = _open(ta, fx)
    try:
        if with_deletes:
            dele = _deleted(fx)
            alive = np.ones(fx.max_doc, bool)
            alive[dele] = False
            dev.set_alive_bitset(_alive_bytes(fx.max_doc, dele))
        want = [FM.tree_expect(L, spec, msm, alive) for spec, msm in cases]
        assert all(w[0].size > 0 for w in want)
        qs = [to_device(ta, spec, msm) for spec, msm in cases]
        ws = [FM.tree_weights(L, spec) for spec, _ in cases]
        exact = [FM.n_scoring(spec) <= 2 and not any(FM.is_phrase(m) for cl in spec for _, m in (cl[1] if isinstance(cl[1], list) else [(M, cl[1])]))
                 for spec, _ in cases]
        dev.set_option("record_query_kernels", 1)
        for k in (1, 10, 100):
            rows = []
            for ex in (0, 1):
                sc, dc, ct = dev.raw_search_trees(qs, ws, L.cache, k, opts=(ex, 0))
                rows.append((_bits(sc).copy(), dc.copy(), ct.copy()))
                assert dev.last_batch_match_counts(len(qs)).tolist() == [w[0].size for w in want], (k, ex)  # the counts
                assert dev.last_batch_query_kernels(len(qs)).tolist() == [KERNEL_TREE] * len(qs)
                for i in range(len(qs)):
                    _check_topk(sc[i], dc[i], ct[i], want[i], k, exact[i], cases[i])
            assert all(np.array_equal(x, y) for x, y in zip(*rows)), k  # "exhaustive" 0 and 1: the same rows, bit for bit
        # tq_count_batch over the same records
        cq, keep = dev._raw_scored_queries(qs, ws, L.cache, 0)
        counts = np.zeros(len(qs), np.uint32)
        assert ta.binding.lib().tq_count_batch(dev.segment_raw(), cq, len(qs), counts.ctypes.data_as(C.POINTER(C.c_uint32))) == 0, _err(ta)
        assert counts.tolist() == [w[0].size for w in want]
        # doc sets under "docset_trees"
        dev.set_option("docset_trees", 1)
        total = sum(w[0].size for w in want)
        rc, docs, starts = dev.raw_docset(qs, total, guard=4)
        assert rc == 0, _err(ta)
        assert np.all(docs[total:] == 0xDEADBEEF)
        for i, w in enumerate(want):
            assert np.array_equal(docs[int(starts[i]): int(starts[i + 1])], w[0]), cases[i]
    finally:
        dev.close()


@pytest.mark.parametrize("with_deletes", [False, True])
def test_standalone_phrases_of_a_non_primary_field(ta, with_deletes):
    fx = FM.fixture_x()
    L = FM.FieldLists(fx)
    alive = None
    dev = _open(ta, fx)
    try:
        if with_deletes:
            dele = _deleted(fx)
            alive = np.ones(fx.max_doc, bool)
            alive[dele] = False
            dev.set_alive_bitset(_alive_bytes(fx.max_doc, dele))
        qs, ws, want = [], [], []
        for pname, terms, offs in PM.QUERIES:
            if pname not in FM.PHRASE_QUERIES:
                continue
            gids = [ABSENT_ID if t == PM.ABSENT else fx.gid(1, t) for t in terms]
            qs.append((O.MODE_PHRASE, gids, list(offs)))
            ws.append([L.phrase_weight(gids)])
            if ABSENT_ID in gids:
                want.append((np.zeros(0, np.uint32), np.zeros(0, np.float32)))
                continue
            present, score = L.phrase(gids, offs)
            if alive is not None:
                present = present & alive
            docs = np.nonzero(present)[0].astype(np.uint32)
            want.append((docs, score[docs]))
        assert len(qs) == len(FM.PHRASE_QUERIES) and sum(1 for w in want if w[0].size) >= 5
        sizes = [w[0].size for w in want]
        assert dev.raw_count(qs, ws, L.cache).tolist() == sizes
        dev.set_option("record_query_kernels", 1)
        for k in (1, 10, 100):
            rows = []
            for ex in (0, 1):
                sc, dc, ct = dev.raw_search(qs, ws, L.cache, k, opts=(ex, 0))
                rows.append((_bits(sc).copy(), dc.copy(), ct.copy()))
                assert dev.last_batch_match_counts(len(qs)).tolist() == sizes, (k, ex)
                assert dev.last_batch_query_kernels(len(qs)).tolist() == [KERNEL_TREE] * len(qs)
                for i in range(len(qs)):
                    _check_topk(sc[i], dc[i], ct[i], want[i], k, False, FM.PHRASE_QUERIES[i])
            assert all(np.array_equal(x, y) for x, y in zip(*rows)), k
        s1, d1, c1 = dev.raw_search_one(qs[0], ws[0], L.cache, 10)
        sc, dc, ct = dev.raw_search(qs[:1], ws[:1], L.cache, 10)
        assert c1 == int(ct[0]) and np.array_equal(d1[:c1], dc[0, :c1]) and np.array_equal(_bits(s1[:c1]), _bits(sc[0, :c1]))
        dev.set_option("docset_trees", 1)
        total = sum(sizes)
        rc, docs, starts = dev.raw_docset(qs, total, guard=4)
        assert rc == 0, _err(ta)
        for i, w in enumerate(want):
            assert np.array_equal(docs[int(starts[i]): int(starts[i + 1])], w[0]), FM.PHRASE_QUERIES[i]
    finally:
        dev.close()


# ---- 4. term sets with members of two fields, beside a term of a third
def test_term_sets_across_fields(ta):
    fx = FM.fixture_x()
    L = FM.FieldLists(fx)
    dev = _open(ta, fx)
    try:
        for g in range(fx.n_terms):  # (every term first: a set's handle then lies above every global term id)
            dev.term_handle(g)
        members = FM.set_members(fx)
        sets = {}
        for weight in (1.0, 2.5):
            h = dev.term_set_prepare(members)
            assert int(h) >= fx.n_terms and dev.term_field(h) == 0
            sets[weight] = FM.add_set(L, h, members, weight)
        assert dev.term_set_info(sets[1.0])[0] == int(L.lists[sets[1.0]][0].sum())
        cases = FM.set_cases(fx, sets[1.0], sets[2.5])
        want, _ = check_cases(ta, dev, L, cases, ks=(1, 10, 100))
        assert all(w[0].size > 0 for w in want)
    finally:
        dev.close()


# ---- 5. tq_term_prepare_batch_fields
def test_prepare_batch_fields(ta):
    fx = FM.fixture_x()
    B = ta.binding
    lib = B.lib()
    dev = _open(ta, fx)
    try:
        seg = dev.segment_raw()
        picks = [(1, 0), (0, 0), (2, 0), (1, 5), (0, 6), (2, 1), (1, 0), (0, 15), (1, 7)]  # (a term named twice; term 0 of every field)
        assert len({fx.fields[f].terms[0].postings_start for f in range(3)}) == 1  # the same postings_off in three fields
        infos = (B.TqTermInfo * len(picks))()
        fields = (C.c_uint8 * len(picks))(*[f for f, _ in picks])
        for i, (f, t) in enumerate(picks):
            ti = fx.fields[f].terms[t]
            infos[i] = B.TqTermInfo(ti.postings_start, ti.positions_start, ti.postings_end - ti.postings_start,
                                    ti.positions_end - ti.positions_start, ti.doc_freq, 0)
        out = (C.c_uint32 * len(picks))()
        assert lib.tq_term_prepare_batch_fields(seg, infos, fields, len(picks), out) == 0, _err(ta)
        hs = list(out)
        assert hs[0] == hs[6] and len(set(hs)) == len(picks) - 1  # one handle per (field, postings_off)
        assert len({hs[0], hs[1], hs[2]}) == 3
        for (f, t), h in zip(picks, hs):
            one, fld = C.c_uint32(), C.c_uint32()
            x = infos[picks.index((f, t))]
            assert lib.tq_term_prepare_field(seg, f, x.postings_off, x.postings_len, x.positions_off, x.positions_len, x.doc_freq, C.byref(one)) == 0
            assert one.value == h
            assert lib.tq_term_field(seg, h, C.byref(fld)) == 0 and fld.value == f
            assert dev.term_handle(fx.gid(f, t)) == h  # the host mirror goes through the same entry points
        out2 = (C.c_uint32 * len(picks))()
        assert lib.tq_term_prepare_batch_fields(seg, infos, fields, len(picks), out2) == 0 and list(out2) == hs
        assert dev.fields_stats() == {"n_fields": 3, "n_field_terms": sum(1 for f, t in set(picks) if f), "extra_fieldnorm_bytes": fx.max_doc}
        # the lists are the fields' own: the device decode of every handle against the oracle's
        for (f, t), h in zip(picks, hs):
            df = fx.fields[f].terms[t].doc_freq
            docs, tfs = np.zeros(df, np.uint32), np.zeros(df, np.uint32)
            assert lib.tq_decode_postings(seg, h, docs.ctypes.data_as(C.POINTER(C.c_uint32)), tfs.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
            wd, wt = O.decode_postings(fx.fields[f], t)
            assert np.array_equal(docs, np.asarray(wd, np.uint32)) and np.array_equal(tfs, np.asarray(wt, np.uint32)), (f, t)
    finally:
        dev.close()


# ---- 6. refusals: nothing is launched, the segment stays usable
def test_refusals_leave_the_segment_usable(ta):
    fx = FM.fixture_x()
    B = ta.binding
    lib = B.lib()
    L = FM.FieldLists(fx)
    dev = _open(ta, fx)
    try:
        seg = dev.segment_raw()
        a, b, b2 = fx.gid(0, 6), fx.gid(1, 0), fx.gid(1, 1)
        for g in (a, b, b2):
            L.need(g)
        # a phrase over two fields
        mixed = [(O.MODE_OR, [b], None), (O.MODE_PHRASE, [a, b], [0, 1])]
        with pytest.raises(B.TantivyAmdError) as e:
            dev.raw_search(mixed, [[1.0], [1.0]], L.cache, 10)
        assert e.value.code == ERR_INVALID and "query 1" in str(e.value) and "different fields" in str(e.value)
        with pytest.raises(B.TantivyAmdError) as e:
            dev.raw_count(mixed, [[1.0], [1.0]], L.cache)
        assert e.value.code == ERR_INVALID and "tq_count_batch: query 1" in str(e.value)
        # a Should term of a field != 0 in a query that a match-all clause makes ALL-BASED (all_kernel knows one norm)
        star = [(O.MODE_OR, [a], None), (ta.MODE_BOOL, [ta.binding.TERM_ALL, b], None, [S, S], None, 0)]
        with pytest.raises(B.TantivyAmdError) as e:
            dev.raw_search(star, [[1.0], [1.0, 1.0]], L.cache, 10)
        assert e.value.code == ERR_UNSUPPORTED and "query 1" in str(e.value)
        assert dev.raw_count(star, [[1.0], [1.0, 1.0]], L.cache).tolist() == [int(L.lists[a][0].sum()), fx.max_doc]  # (its count is taken)
        dev.set_option("docset_trees", 1)
        rc, _, _ = dev.raw_docset([(O.MODE_OR, [b]), (O.MODE_PHRASE, [a, b], [0, 1])], 1 << 14)
        assert rc == ERR_INVALID and b"query 1" in _err(ta)
        atom = to_device(ta, [(M, b2), (M, ("ph", [a, b]))], 0)  # ... as a phrase atom
        with pytest.raises(B.TantivyAmdError) as e:
            dev.raw_search_trees([atom], [[1.0, 1.0, 1.0]], L.cache, 10)
        assert e.value.code == ERR_INVALID and "query 0" in str(e.value)
        # a field the segment does not have
        h = C.c_uint32()
        ti = fx.fields[0].terms[0]
        assert lib.tq_term_prepare_field(seg, 3, ti.postings_start, ti.postings_end - ti.postings_start, 0, 0, ti.doc_freq, C.byref(h)) == ERR_INVALID
        info = (B.TqTermInfo * 1)(B.TqTermInfo(ti.postings_start, 0, ti.postings_end - ti.postings_start, 0, ti.doc_freq, 0))
        assert lib.tq_term_prepare_batch_fields(seg, info, (C.c_uint8 * 1)(5), 1, C.byref(h)) == ERR_INVALID
        # 0 fields, more than TQ_MAX_FIELDS
        idx = np.ascontiguousarray(fx.fields[0].idx[: fx.fields[0].idx_len])
        ff = (B.TqFieldFiles * 9)(*[B.TqFieldFiles(idx.ctypes.data, idx.size, None, 0, None, 0) for _ in range(9)])
        for n in (0, 9):
            s2 = C.c_void_p()
            assert lib.tq_segment_upload_fields(dev.ctx, 0, fx.max_doc, n, ff, fx.fields[0].record_option, C.byref(s2)) == ERR_INVALID
            assert not s2.value
        # the scored doc set of a multi-field tree: not in this version
        dev.set_option("docset_score_trees", 1)
        tree = to_device(ta, [(M, a), (M, [(M, b), (M, b2)], 0)], 0)
        rc, _, _, _ = dev.raw_docset_scored([(O.MODE_OR, [a]), tree], 1 << 14, weights=[[1.0], [1.0, 1.0, 1.0]], cache=L.cache)
        assert rc == ERR_UNSUPPORTED and b"query 1" in _err(ta)
        # the next valid batch gives the right rows
        want, _ = check_cases(ta, dev, L, [([(M, T(a)), (M, T(b))], 0), ([(S, T(b)), (S, T(b2))], 0)], ks=(10,))
        assert all(w[0].size > 0 for w in want)
    finally:
        dev.close()


# ---- 7. the host mirror through DeviceIndex.add_segment_fields
def test_host_mirror_equals_the_raw_rows(ta):
    from tests.test_gpu_all import _entries, _weights_of

    fx = FM.fixture_x()
    L = FM.FieldLists(fx)
    cases = FM.flat_cases(fx)[5:9]  # the parser's shapes, with and without a MustNot of another field
    dev = _open(ta, fx)
    try:
        hostq, srch, flat, ws = [], [], [], []
        for c, m in cases:
            t, o, cof, whats = _entries(c)
            for g in t:
                L.need(g)
            hostq.append((ta.MODE_BOOL, t, o, cof, m))
            flat.append((ta.MODE_BOOL, t, o, cof, m))
            srch.append((ta.MODE_BOOL, t, None, o, cof, m))
            ws.append(_weights_of(whats, L))
        k = 10
        sc, dc, ct = dev.raw_search(srch, ws, L.cache, k)
        hs, ho, hd, hc = dev.search(hostq, k)
        assert np.array_equal(hc, ct) and np.array_equal(hd, dc) and np.all(ho[hd != TERMINATED] == 0)
        assert np.array_equal(_bits(hs), _bits(sc))
        counts = dev.raw_count(srch, ws, L.cache)
        assert dev.count(hostq).tolist() == counts.tolist()
        total = int(counts.sum())
        rc, docs, starts = dev.raw_docset(flat, total)
        assert rc == 0, _err(ta)
        rc, sdocs, scores, sstarts = dev.raw_docset_scored(flat, total, weights=ws, cache=L.cache)
        assert rc == 0, _err(ta)
        hsets, hscored = dev.docset(hostq), dev.docset_scored(hostq)
        for i in range(len(cases)):
            a, b = int(starts[i]), int(starts[i + 1])
            assert np.array_equal(hsets[i][:, 1], docs[a:b]) and np.all(hsets[i][:, 0] == 0)
            assert np.array_equal(hscored[i][0][:, 1], sdocs[a:b]) and np.array_equal(_bits(hscored[i][1]), _bits(scores[a:b]))
        # Query::phrase over terms of different fields: InvalidArgument
        with pytest.raises(ta.binding.TantivyAmdError) as e:
            dev.search([(ta.MODE_PHRASE, [fx.gid(0, 6), fx.gid(1, 0)], [0, 1])], k)
        assert e.value.code == ERR_INVALID
    finally:
        dev.close()
