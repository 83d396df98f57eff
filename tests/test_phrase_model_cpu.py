"""The plain phrase model (tests/phrase_model.py) against the C oracle on every corpus and query of
tests/test_gpu_phrase_positions.py, and the conditions on those inputs that the GPU tests rely on — every listed edge
is looked up in the SERIALISED segment (decoded postings and position deltas), so that a GPU test cannot pass because
its corpus missed the edge.  Runs without a GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import phrase_model as PM
from tests.helpers import rel_close


@pytest.fixture(scope="module", params=PM.CORPORA)
def corp(request):
    return PM.corpus(request.param)


def _qi(name):
    return [q[0] for q in PM.QUERIES].index(name)


def _layout(seg, t):
    """Term t's position stream as serialised: (deltas, {doc: (index of its first delta, tf)}, widths of the bitpacked
    blocks, length of the vint tail)."""
    docs, tfs = O.decode_postings(seg, t)
    total = int(tfs.sum())
    positions, n = O.decode_positions(seg, t, total)  # (absolute within each doc)
    assert n == total
    starts = np.concatenate([[0], np.cumsum(tfs.astype(np.int64))[:-1]]).astype(np.int64)
    deltas = positions.astype(np.int64)
    deltas[1:] -= positions[:-1]
    deltas[starts] = positions[starts]
    assert deltas.min() >= 0
    runs = {int(d): (int(s), int(f)) for d, s, f in zip(docs, starts, tfs)}
    n_pb = total // 128
    widths = [int(deltas[128 * b: 128 * b + 128].max()).bit_length() for b in range(n_pb)]
    return deltas, runs, widths, total - 128 * n_pb


# ---------------------------------------------------------------------------------------------- model == oracle
def test_model_matches_oracle_and_literal_merge(corp):
    seg = corp.segment()
    for qi, (name, terms, offs) in enumerate(corp.queries):
        docs, scores, counts = corp.expect(qi)
        merged = PM.phrase_counts_merge(corp.tp, terms, offs, corp.alive)
        assert merged == {int(d): int(c) for d, c in zip(docs, counts)}, name
        if name == "absent":  # (the oracle takes terms of the segment only)
            assert docs.size == 0
            continue
        od, osc = O.match_all(seg, terms, O.MODE_PHRASE, phrase_offsets=offs)
        if corp.alive is not None:
            keep = corp.alive[od]
            od, osc = od[keep], osc[keep]
        assert np.array_equal(od, docs), (corp.name, name, od[:8], docs[:8], od.size, docs.size)
        for d, a, b in zip(docs, osc, scores):
            assert rel_close(float(a), float(b), 1e-5), (corp.name, name, int(d), float(a), float(b))


def test_term_order_does_not_change_counts(corp):
    """min-multiplicity is symmetric in the terms; the sequential merges are checked to be, too."""
    for name in ("p3", "p4", "aba"):
        _, terms, offs = corp.queries[_qi(name)]
        want = PM.phrase_counts(corp.tp, terms, offs, corp.alive)
        for perm in ([1, 0] + list(range(2, len(terms))), list(range(len(terms)))[::-1]):
            t2, o2 = [terms[i] for i in perm], [offs[i] for i in perm]
            assert PM.phrase_counts_merge(corp.tp, t2, o2, corp.alive) == want, (name, perm)


# ---------------------------------------------------------------------------------------------- input conditions
def test_inputs_cannot_pass_vacuously(corp):
    assert 4096 <= corp.max_doc <= 70_000 and len(corp.tp) <= 10
    assert max(corp.fieldnorms) <= 40
    table = O.fieldnorm_table()
    for f in set(corp.fieldnorms):
        assert int(table[O.fieldnorm_to_id(f)]) == f
    dfs = corp.dfs()
    assert dfs[0] < min(dfs[1:]) or corp.name == "P"  # (P: terms 2 and 3 are short on purpose)
    docs, scores, counts = corp.expect(PM.MAIN)
    assert docs.size >= 20 and int((counts >= 2).sum()) >= 5
    _, terms, offs = corp.queries[PM.MAIN]
    near = PM.near_misses(corp.tp, terms, offs, corp.alive)  # every term, the second one exactly one position late
    assert len(near) >= 20, len(near)
    avgdl = sum(corp.fieldnorms) / corp.max_doc
    for qi, (name, terms, offs) in enumerate(corp.queries):
        d, s, c = corp.expect(qi)
        assert d.size <= 1000, (name, d.size)
        if name in ("nomatch", "absent"):
            assert d.size == 0
        else:
            assert d.size >= 1, name
            assert len(PM.and_docs(corp.tp, terms, corp.alive)) > d.size, name  # the AND is larger than the phrase
            assert int(c.max()) <= 40
            w = PM.phrase_weight(corp.tp, terms, corp.max_doc)
            for dl in set(corp.fieldnorms):
                assert PM.min_relative_gap(w, range(1, int(c.max()) + 1), dl, avgdl) >= 10 * 1e-5


def _matching_runs(corp, names):
    """{term: [(start, tf, doc)]} of the runs of the docs that match one of the named queries, per term of the query."""
    seg = corp.segment()
    lay = {}
    out = {}
    for name in names:
        qi = _qi(name)
        _, terms, _ = corp.queries[qi]
        for d in corp.expect(qi)[0]:
            for t in set(terms):
                if t not in lay:
                    lay[t] = _layout(seg, t)
                s, f = lay[t][1][int(d)]
                out.setdefault(t, []).append((s, f, int(d)))
    return out, lay


def test_P_edges_are_in_the_serialised_stream():
    corp = PM.corpus("P")
    runs, lay = _matching_runs(corp, ["p2", "rev2", "p4"])
    assert lay[0][2] == PM.P_WIDTHS0 and lay[1][2] == PM.P_WIDTHS1
    assert 0 < lay[0][3] < 128 and 0 < lay[1][3] < 128
    for t in (0, 1):  # leader and non-leader of "0 1"
        _, _, widths, tail = lay[t]
        n_pb = len(widths)
        touched, ends_127, starts_127, into_tail, in_tail = set(), 0, 0, 0, 0
        for s, f, _ in runs[t]:
            e = s + f - 1
            for b in range(s >> 7, (e >> 7) + 1):
                if b < n_pb:
                    touched.add(widths[b])
            ends_127 += (e >> 7) < n_pb and (e & 127) == 127 and f >= 2
            starts_127 += (s & 127) == 127 and f >= 2 and (e >> 7) < n_pb
            into_tail += (s >> 7) == n_pb - 1 and (e >> 7) == n_pb
            in_tail += (s >> 7) == n_pb
        assert touched >= {0, 1, 7, 8, 9, 16, 31, 32}, (t, touched)
        assert ends_127 >= 1 and starts_127 >= 1 and into_tail >= 1 and in_tail >= 1, (t, ends_127, starts_127, into_tail, in_tail)
    deltas0 = lay[0][0]
    assert int(deltas0.max()) >= 1 << 31 and int(deltas0.max()) + 8 + 100000 < 1 << 32
    # term 2: no bitpacked block; term 3: exactly two, no tail; both hold matching docs, term 3's on both sides of its edge
    assert lay[2][2] == [] and 0 < lay[2][3] < 128
    assert len(lay[3][2]) == 2 and lay[3][3] == 0
    assert {s >> 7 for s, _, _ in runs[3]} == {0, 1}
    assert corp.expect(_qi("p3"))[0].size >= 10 and corp.expect(_qi("p4"))[0].size >= 10


@pytest.mark.parametrize("name", ["T", "T2"])
def test_T_edges_are_in_the_serialised_postings(name):
    corp = PM.corpus(name)
    seg = corp.segment()
    match = {int(d): int(c) for d, c in zip(corp.expect(PM.MAIN)[0], corp.expect(PM.MAIN)[2])}
    post = {}
    for t in (0, 1):
        docs, tfs = O.decode_postings(seg, t)
        post[t] = (docs.tolist(), tfs.tolist(), {int(d): i for i, d in enumerate(docs)})
    seen = set()
    for big, tf, d in corp.notes["small"]:
        docs, tfs, at = post[big]
        assert tfs[at[d]] == tf and 1 <= match[d] <= 2
        assert 1 <= post[1 - big][1][post[1 - big][2][d]] <= 2
        seen.add((big, tf))
    assert seen == {(b, tf) for b in (0, 1) for tf in PM.T_SMALL_TFS}
    assert [(tf, match[d]) for tf, d in corp.notes["both"]] == [(tf, tf) for tf in PM.T_SMALL_TFS for _ in range(2)]
    seen = set()
    for big, tf, slot, d in corp.notes["big"]:
        docs, tfs, at = post[big]
        i = at[d]
        assert tfs[i] == tf and i & 3 == slot and match[d] == 2
        assert docs[i + 1] == d + 1 and match[d + 1] == 1  # the next posting is a match, too ...
        seen.add((big, tf, slot, (i + 1) & 3 != 0))       # ... in the same group unless the slot is 3
    assert {s[:3] for s in seen} == {(b, tf, s) for b in (0, 1) for tf in PM.T_BIG_TFS for s in range(4)}
    assert all(s[3] == (s[2] < 3) for s in seen)
    if name == "T2":  # every k the pruned runs ask for (1, 3, 10) cuts through a tie
        d, s, c = corp.expect(PM.MAIN)
        top = np.sort(s)[::-1]
        assert len(set(corp.fieldnorms)) == 2
        assert top[0] == top[1] and top[2] == top[3] and top[9] == top[10]
        assert top[1] > top[2] and top[3] > top[4]
        assert np.unique(s).size < s.size // 2


def test_R_shapes_are_present():
    corp = PM.corpus("R")
    c2 = dict(zip(corp.expect(_qi("p2"))[0].tolist(), corp.expect(_qi("p2"))[2].tolist()))
    c3 = dict(zip(corp.expect(_qi("p3"))[0].tolist(), corp.expect(_qi("p3"))[2].tolist()))
    seen = set()
    dfs = corp.dfs()
    assert dfs[0] < min(dfs[1:])
    for name, long_term, d, want2, want3 in corp.notes["rep"]:
        assert c2[d] == want2 and c3[d] == want3, (name, long_term, d)
        mult = tuple(max(np.unique(corp.tp[t][d], return_counts=True)[1]) for t in range(3))
        tf = tuple(len(corp.tp[t][d]) for t in range(3))
        assert long_term is None or tf[long_term] == 9
        assert max(tf) <= (3 if long_term is None else 9)
        seen.add((mult, long_term))
    for mult in ((2, 1, 1), (2, 2, 1), (1, 2, 1), (2, 3, 1), (2, 3, 2)):
        for long_term in (None, 0, 1):
            assert (mult, long_term) in seen, (mult, long_term)


@pytest.mark.parametrize("name", ["D", "Ddel"])
def test_D_placement(name):
    corp = PM.corpus(name)
    seg = corp.segment()
    docs = set(corp.expect(PM.MAIN)[0].tolist())
    lead_docs, _ = O.decode_postings(seg, 0)
    assert lead_docs.size > 8192
    edge = list(PM.D_EDGE_DOCS) + [int(lead_docs[127]), int(lead_docs[128])]
    assert (int(lead_docs[127]), int(lead_docs[128])) == corp.notes["lead_127_128"]
    if corp.deleted is None:
        assert all(d in docs for d in edge)
        assert any(d in docs for d in lead_docs[8192:].tolist())  # a match in the second 64-block tile
    else:
        assert len(corp.deleted) == corp.max_doc // 3
        assert not docs & set(corp.deleted)
        full = set(PM.corpus("D").expect(PM.MAIN)[0].tolist())
        assert docs == {d for d in full if corp.alive[d]} and len(docs) < len(full)
