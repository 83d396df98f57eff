"""Every device path that decides a phrase match, against the plain model of tests/phrase_model.py (token-level
positions -> min-multiplicity counts -> float64 BM25), on corpora built for the edges of the position codec, the term
freq hand-overs, repeated positions and doc placement (tests/test_phrase_model_cpu.py proves on the CPU that the
corpora hold those edges and that the model is the oracle's and the reference's semantics).

Paths (tantivy_amd/csrc): 1 phrase_kernel<DENSE=false> ("use_dense" 0; phrases of up to 4 terms in a batch of their own, so
that the 4-term instantiation with the register path runs, 5 and 8 terms in a second one), 2 phrase_kernel<DENSE=true> (leader without
tables, every other list with them), 3 + 4 phrase_sweep_kernel's register path and cursor merge (all lists with tables),
5 the phrase atoms of tq_tree.hip, 6 those of tq_docset_tree.hip ("docset_trees").  Each configuration asserts the
kernel bit that ran.  Docs are exact everywhere; a score within 1e-5 of the model's pins the phrase count (the CPU test
asserts a gap of >= 1e-4 between the scores of neighbouring counts)."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import phrase_model as PM
from tests.helpers import alive_bytes, exhaustive_by_default

pytestmark = pytest.mark.gpu

K_ALL = 1024  # every query has <= 1000 matches (asserted on the CPU): the exhaustive top-1024 is the full set
M = O.MUST
PH = 0x10  # TQ_NESTED_PHRASE
EXTRA = 7  # the term of `+"..." +c`


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return exhaustive_by_default(tantivy_amd)


def _open(ta, corp, options):
    dev = ta.DeviceIndex([corp.segment()])
    try:
        dev.set_option("dense_budget_x", 256)  # (small segments: the tables of every list that qualifies fit)
        for name, value in options:
            dev.set_option(name, value)
        dev.set_option("record_query_kernels", 1)
        if corp.deleted is not None:
            dev.set_alive_bitset(alive_bytes(corp.max_doc, corp.deleted))
    except Exception:
        dev.close()
        raise
    return dev


def _dense(corp, t, ratio):
    return corp.max_doc >= 4096 and corp.dfs()[t] * ratio >= corp.max_doc


def _by_df(corp, terms):
    return sorted(terms, key=lambda t: corp.dfs()[t])


def _lean_ratio(corp):
    """"dense_ratio" under which term 1 has tables and term 0 has none."""
    dfs = corp.dfs()
    r = -(-corp.max_doc // dfs[1])
    assert dfs[0] * r < corp.max_doc <= dfs[1] * r
    return r


def _lean_ok(corp, terms, ratio):
    """route_phrase's stated conditions for the lean instantiation (phrase_kernel<DENSE=true>): at most 4 terms, every
    non-leader list with a bitmap, a doc-matrix column, tf bytes and a position directory — and not the sweep, which
    needs the leader's tables as well.  The kernel mask cannot tell path 1 from path 2 (both are KERNEL_PHRASE), so the
    batch of that configuration holds ONLY queries chosen by this rule: one query outside it sends the whole launch
    group to the general instantiation."""
    if len(terms) > 4 or any(t >= PM.NT for t in terms):
        return False
    order = _by_df(corp, terms)
    return not _dense(corp, order[0], ratio) and all(_dense(corp, t, ratio) for t in order[1:])


def _sweeps(corp, terms, ratio):
    order = _by_df(corp, terms)
    return (len(terms) <= 4 and all(_dense(corp, t, ratio) for t in terms)
            and corp.dfs()[order[0]] * 128 >= corp.max_doc)


def _rows(res, n):
    scores, _, docs, counts = res
    out = []
    for i in range(n):
        c = int(counts[i])
        assert np.all(docs[i, c:] == 0x7FFFFFFF)
        out.append((scores[i, :c].copy(), docs[i, :c].copy()))
    return out


def _assert_model(corp, name, got_scores, got_docs, want_docs, want_scores):
    """got: a full result row in rank order; want: the model's (docs ascending, float64 scores)."""
    ws, wd = PM.top_k(want_docs, want_scores, K_ALL)
    assert got_docs.size == wd.size and np.array_equal(got_docs, wd), (corp.name, name, got_docs[:10], wd[:10], got_docs.size, wd.size)
    rel = np.abs(got_scores.astype(np.float64) - ws) / np.maximum(np.abs(ws), 1e-30)
    assert np.all(rel <= 1e-5), (corp.name, name, got_docs[rel > 1e-5][:8], got_scores[rel > 1e-5][:8], ws[rel > 1e-5][:8])


def _oracle_rows(corp, terms, offs):
    od, osc = O.match_all(corp.segment(), terms, O.MODE_PHRASE, phrase_offsets=offs)
    if corp.alive is not None:
        keep = corp.alive[od]
        od, osc = od[keep], osc[keep]
    order = np.lexsort((od, -osc.astype(np.float64)))
    return osc[order], od[order]


def _assert_pruned(dev, queries, full):
    """"exhaustive" 0: the arrays of the exhaustive run cut to k — the model's top-k with ties to the lower doc."""
    dev.set_option("exhaustive", 0)
    try:
        for k in (1, 3, 10):
            got = _rows(dev.search(queries, k), len(queries))
            for qi, ((gs, gd), (fs, fd)) in enumerate(zip(got, full)):
                assert np.array_equal(gd, fd[:k]) and np.array_equal(gs, fs[:k]), (k, qi, gd, fd[:k], gs, fs[:k])
    finally:
        dev.set_option("exhaustive", 1)


FLAT = ["sparse", "lean", "sweep"]


def _flat_batches(corp, config):
    """-> (options, "dense_ratio" or None, [batch of query indices]).  launch_phrase_t picks ONE instantiation per
    launch group from the group's largest query: the phrases of up to 4 terms go in a batch of their own wherever their
    instantiation (phrase_kernel<KPL, 4, DENSE>: the register path, pos_run_delta) is what the configuration is about."""
    every = list(range(len(corp.queries)))
    short = [qi for qi in every if len(corp.queries[qi][1]) <= 4]
    long_ = [qi for qi in every if len(corp.queries[qi][1]) > 4]
    if config == "sparse":  # path 1: <4, false> for the short batch, <8, false> (cursor merge only) for p5 / p8
        return [("use_dense", 0)], None, [short, long_]
    if config == "lean":  # path 2
        ratio = _lean_ratio(corp)
        picked = [qi for qi in every if _lean_ok(corp, corp.queries[qi][1], ratio)]
        assert PM.MAIN in picked and len(picked) >= 2
        return [("dense_ratio", ratio)], ratio, [picked]
    # paths 3 and 4: the 5- and 8-term phrases of the same batch are the whole leftover phrase group (<8, false>)
    assert all(_dense(corp, t, 128) for t in range(PM.NT))
    return [("dense_ratio", 128)], 128, [every]


@pytest.mark.parametrize("config", FLAT)
@pytest.mark.parametrize("name", PM.CORPORA)
def test_flat_phrases(ta, name, config):
    corp = PM.corpus(name)
    B = ta.binding
    options, ratio, batches = _flat_batches(corp, config)
    dev = _open(ta, corp, options)
    try:
        used = set()
        for picked in batches:
            queries = [(O.MODE_PHRASE, corp.queries[qi][1], corp.queries[qi][2]) for qi in picked]
            full = _rows(dev.search(queries, K_ALL), len(queries))
            kern = dev.last_batch_query_kernels(len(queries))
            counts = dev.last_batch_match_counts(len(queries))
            used |= {t for qi in picked for t in corp.queries[qi][1] if t < PM.NT}
            if ratio is not None:  # every list that qualifies has its bitmap AND its doc-matrix column (route_phrase's `col`)
                st = dev.segment_stats(0)
                n_dense = sum(_dense(corp, t, ratio) for t in used)
                assert st["n_dense_lists"] == n_dense and st["n_docmat_columns"] == n_dense, st
            n_sweep = 0
            for at, qi in enumerate(picked):
                qname, terms, offs = corp.queries[qi]
                wd, ws, wc = corp.expect(qi)
                _assert_model(corp, qname, full[at][0], full[at][1], wd, ws)
                assert int(counts[at]) == wd.size, (qname, int(counts[at]), wd.size)
                if qname == "absent":
                    continue
                want_kernel = B.KERNEL_PHRASE_SWEEP if config == "sweep" and _sweeps(corp, terms, ratio) else B.KERNEL_PHRASE
                assert int(kern[at]) == want_kernel, (qname, B.kernel_names(int(kern[at])))
                n_sweep += want_kernel == B.KERNEL_PHRASE_SWEEP
                os_, od = _oracle_rows(corp, terms, offs)  # bit-equal to the oracle, as tests/test_gpu_parity.py::test_phrase
                assert np.array_equal(od, full[at][1]) and np.array_equal(os_.view(np.uint32), full[at][0].view(np.uint32)), qname
            if config == "sweep":
                by_name = {corp.queries[qi][0]: int(kern[at]) for at, qi in enumerate(picked)}
                assert n_sweep >= 8 and by_name["p5"] == B.KERNEL_PHRASE and by_name["p8"] == B.KERNEL_PHRASE
            _assert_pruned(dev, queries, full)
    finally:
        dev.close()


def _as_clause(terms, offs, extra=None):
    """The phrase as the only Must clause of a boolean query, or `+"..." +extra`."""
    n = len(terms)
    if extra is None:
        return (O.MODE_BOOL, list(terms), [M] * n, [0] * n, 0,
                {"nested_occurs": [M | PH] * n, "atom_of": [0] * n, "phrase_offsets": list(offs)})
    return (O.MODE_BOOL, list(terms) + [extra], [M] * (n + 1), [0] * n + [1], 0,
            {"nested_occurs": [M | PH] * n + [M], "atom_of": [0] * (n + 1), "phrase_offsets": list(offs) + [0]})


def _term_scores(corp, t, docs):
    """float64 BM25 of the single term t on `docs`."""
    n = len(corp.tp[t])
    w = (1.0 + PM.K1) * math.log(1.0 + (corp.max_doc - n + 0.5) / (n + 0.5))
    avgdl = sum(corp.fieldnorms) / corp.max_doc
    return np.array([PM.bm25(w, len(corp.tp[t][int(d)]), float(corp.fieldnorms[int(d)]), avgdl) for d in docs], np.float64)


@pytest.mark.parametrize("name", PM.CORPORA)
def test_phrase_atoms_of_the_tree_kernel(ta, name):
    corp = PM.corpus(name)
    B = ta.binding
    nq = len(corp.queries)
    queries = [_as_clause(terms, offs) for _, terms, offs in corp.queries]
    queries += [_as_clause(terms, offs, EXTRA) for _, terms, offs in corp.queries]
    dev = _open(ta, corp, [])
    try:
        full = _rows(dev.search(queries, K_ALL), len(queries))
        kern = dev.last_batch_query_kernels(len(queries))
        counts = dev.last_batch_match_counts(len(queries))
        n_both = 0
        for qi, (qname, terms, offs) in enumerate(corp.queries):
            wd, ws, _ = corp.expect(qi)
            _assert_model(corp, qname, full[qi][0], full[qi][1], wd, ws)
            has = np.array([int(d) in corp.tp[EXTRA] for d in wd], bool)
            wd2 = wd[has]
            ws2 = ws[has] + _term_scores(corp, EXTRA, wd2)
            _assert_model(corp, qname + " +c", full[nq + qi][0], full[nq + qi][1], wd2, ws2)
            assert int(counts[qi]) == wd.size and int(counts[nq + qi]) == wd2.size, qname
            n_both += wd2.size
            if qname != "absent":
                assert int(kern[qi]) == B.KERNEL_TREE and int(kern[nq + qi]) == B.KERNEL_TREE, (qname, kern[qi], kern[nq + qi])
        assert n_both >= 20
        _assert_pruned(dev, queries, full)
    finally:
        dev.close()


@pytest.mark.parametrize("name", PM.CORPORA)
def test_docsets_and_counts(ta, name):
    corp = PM.corpus(name)
    B = ta.binding
    queries = [(O.MODE_PHRASE, terms, offs) for _, terms, offs in corp.queries]
    dev = _open(ta, corp, [("docset_trees", 1)])
    try:
        got = dev.docset(queries)
        st = dev.last_batch_stats()
        assert st["kernel_mask"] & B.KERNEL_DOCSET_TREE, st
        for qi, (qname, _, _) in enumerate(corp.queries):
            wd = corp.expect(qi)[0]
            assert np.all(got[qi][:, 0] == 0)
            assert np.array_equal(got[qi][:, 1], wd), (qname, got[qi][:8, 1], wd[:8], got[qi].shape[0], wd.size)
        assert np.array_equal(dev.count(queries), np.array([corp.expect(qi)[0].size for qi in range(len(queries))], np.uint64))
    finally:
        dev.close()
