"""Multi-field segments (include/tantivy_amd.h "multi-field segments"): the fixtures of tests/test_fields_cpu.py and
tests/test_gpu_fields.py and the glue between them and the models.  Nothing here comes from the product.

Every field is an oracle segment (O.build_segment, or a tests/phrase_model.py corpus's .segment()); a term of the
fixture is a GLOBAL id, assigned field by field in order (DeviceIndex.add_segment_fields does the same).  Doc sets and tfs
come from O.decode_postings, per-list scores from O.bm25_for_one_term / O.bm25_score under THAT field's average fieldnorm
and THAT field's fieldnorm ids, boolean results from tests/all_model.py over `lists` keyed by the global id, phrase
counts and scores from tests/phrase_model.py over the field's own token positions and fieldnorms.

FieldLists(fx, as_primary=True) is the same model with field 0's fieldnorms and cache for EVERY term: what a kernel that
ignores the field tag computes.  tests/test_fields_cpu.py shows that it differs on every scored case."""
import functools
import types

import numpy as np

from oracle import oracle as O
from tests import all_model as AM
from tests import phrase_model as PM

S, M, N = AM.SHOULD, AM.MUST, AM.MUST_NOT
F32 = np.float32


class Fixture:
    """fields: oracle segments over one doc-id space; tps[f]: the field's token positions (phrase_model form) or None."""

    def __init__(self, name, fields, tps, fn_values):
        self.name, self.fields, self.tps, self.fn_values = name, fields, tps, fn_values
        self.max_doc = fields[0].max_doc
        assert all(f.max_doc == self.max_doc and f.record_option == fields[0].record_option for f in fields)
        self.bases = [0]
        for f in fields:
            self.bases.append(self.bases[-1] + len(f.terms))
        self.n_terms = self.bases[-1]

    def gid(self, field, t):
        assert 0 <= t < len(self.fields[field].terms)
        return self.bases[field] + t

    def field_of(self, gid):
        for f in range(len(self.fields)):
            if self.bases[f] <= gid < self.bases[f + 1]:
                return f, gid - self.bases[f]
        raise KeyError(gid)

    def avg(self, f):
        seg = self.fields[f]
        return float(F32(seg.total_num_tokens) / F32(seg.max_doc))

    def fn_ids(self, f):
        """The fieldnorm id of every doc under field f (no fieldnorm file: the constant id 1)."""
        seg = self.fields[f]
        return np.ones(self.max_doc, np.uint8) if seg.fieldnorm is None else np.asarray(seg.fieldnorm, np.uint8)

    def caches(self):
        """tq_query.tf_cache of the fixture: row f = Bm25Weight.cache under field f's average fieldnorm."""
        return np.stack([np.array(list(O.bm25_for_one_term(1, self.max_doc, self.avg(f)).cache), F32)
                         for f in range(len(self.fields))])


def _list_scores(seg, t, max_doc, avg, fn_ids):
    """(present, score, weight) of one list: oracle decode, oracle BM25 per (fieldnorm id, tf) pair."""
    docs, tfs = O.decode_postings(seg, t)
    docs, tfs = np.asarray(docs, np.int64), np.asarray(tfs, np.int64)
    w = O.bm25_for_one_term(seg.terms[t].doc_freq, max_doc, avg)
    ids = fn_ids[docs].astype(np.int64)
    pairs, inverse = np.unique(ids * (1 << 32) + tfs, return_inverse=True)
    table = np.array([O.bm25_score(w, int(p >> 32), int(p & 0xFFFFFFFF)) for p in pairs], F32)
    present = np.zeros(max_doc, bool)
    score = np.zeros(max_doc, F32)
    present[docs] = True
    score[docs] = table[inverse]
    return present, score, float(w.weight)


class FieldLists:
    """tests/test_gpu_all.Lists over a multi-field fixture (seg / lists / weights / cache / need), keyed by global id."""

    def __init__(self, fx, as_primary=False):
        self.fx, self.as_primary = fx, as_primary
        self.seg = types.SimpleNamespace(max_doc=fx.max_doc, terms=[None] * fx.n_terms)
        self.lists, self.weights = {}, {}
        self.cache = fx.caches()

    def _norm_field(self, f):
        return 0 if self.as_primary else f

    def need(self, g):
        if g in self.lists or not isinstance(g, (int, np.integer)) or g >= self.fx.n_terms:
            return
        f, t = self.fx.field_of(g)
        nf = self._norm_field(f)
        p, s, w = _list_scores(self.fx.fields[f], t, self.fx.max_doc, self.fx.avg(nf), self.fx.fn_ids(nf))
        self.lists[g], self.weights[g] = (p, s), w

    def phrase_weight(self, gids):
        """Bm25Weight::for_terms over the phrase's terms: (1 + K1) * the sum of their idfs, as the caller passes it."""
        f = self.fx.field_of(gids[0])[0]
        dfs = [self.fx.fields[f].terms[self.fx.field_of(g)[1]].doc_freq for g in gids if g < self.fx.n_terms]
        return float(O.bm25_for_terms(dfs, self.fx.max_doc, self.fx.avg(f)).weight)

    def phrase(self, gids, offsets):
        """(present, f32 score) of a phrase of ONE field from tests/phrase_model.py: counts from the field's token
        positions, scores from the definition (float64) under the field's fieldnorm values."""
        fl = [self.fx.field_of(g) for g in gids]
        f = fl[0][0]
        assert all(x[0] == f for x in fl), "a phrase is of one field"
        nf = self._norm_field(f)
        docs, sc, _ = PM.phrase_scores(self.fx.tps[f], [t for _, t in fl], list(offsets), self.fx.fn_values[nf])
        present = np.zeros(self.fx.max_doc, bool)
        score = np.zeros(self.fx.max_doc, F32)
        present[docs] = True
        score[docs] = sc.astype(F32)
        return present, score


def is_phrase(x):
    return isinstance(x, tuple) and len(x) >= 2 and x[0] == "ph"


def tree_expect(L, spec, msm=0, alive=None):
    """Ascending (docs, scores) of a tests/tree_shapes.py spec over global ids (term clauses, nested BooleanQuerys of terms
    and phrases, phrases ("ph", [ids]) with offsets 0..n-1): every nested query is one complex_scorer whose result enters
    the outer one as a list.  (A nested result's cost is its size here, its cheapest member's doc freq in the reference:
    the order of an intersection of TWO is immaterial, f32 addition being commutative, and no spec of these tests has more
    than two Must clauses on the outer level.)"""
    lists = dict(L.lists)
    n = L.fx.max_doc

    def leaf(x):
        if is_phrase(x):
            key = ("ph",) + tuple(x[1])
            if all(g < L.fx.n_terms for g in x[1]):
                lists[key] = L.phrase(x[1], range(len(x[1])))
                return ("term", key)
            return ("absent",)
        L.need(x)
        if x in L.lists:
            lists[x] = L.lists[x]
            return ("term", x)
        return ("absent",)

    assert sum(1 for cl in spec if cl[0] == M) <= 2
    clauses = []
    for i, cl in enumerate(spec):
        if isinstance(cl[1], list):
            inner = [(io, leaf(m)) for io, m in cl[1]]
            sc, _ = AM.complex_scorer(inner, cl[2] if len(cl) > 2 else 0, lists, n)
            lists[("nested", i)] = (sc.present, sc.score)
            clauses.append((cl[0], ("term", ("nested", i))))
        else:
            clauses.append((cl[0], leaf(cl[1])))
    return AM.expect(clauses, msm, lists, n, alive)


def n_scoring(spec):
    k = 0
    for cl in spec:
        if cl[0] == N:
            continue
        for io, m in (cl[1] if isinstance(cl[1], list) else [(M, cl[1])]):
            k += 0 if io == N else (len(m[1]) if is_phrase(m) else 1)
    return k


def tree_weights(L, spec):
    """The weights of tree_shapes.to_device(spec)'s entries, in its order: a term's own, a phrase's on each of its terms."""
    out = []
    for cl in spec:
        for _, m in (cl[1] if isinstance(cl[1], list) else [(M, cl[1])]):
            if is_phrase(m):
                out += [L.phrase_weight(m[1])] * len(m[1])
            else:
                L.need(m)
                out.append(L.weights.get(m, 1.0))
    return out


def differs(a, b):
    """The discrimination rule: another top-k doc sequence, or a score off by more than 1e-3 relative."""
    (da, sa), (db, sb) = a, b
    if not np.array_equal(da, db):
        return True
    ta_, tb = AM.top_k(da, sa, 10), AM.top_k(db, sb, 10)
    if not np.array_equal(ta_[1], tb[1]):
        return True
    return bool(np.any(np.abs(sa - sb) > 1e-3 * np.abs(sa)))


# ------------------------------------------------------------------------------------------------ the fixtures
X_DFS0 = [1, 128, 129, 100, 60, 30, 2000, 1500, 700, 300, 256, 500, 47, 46, 1000, 3000]


def _random_field(rng, max_doc, dfs, fn_ids, forced=(), total_num_tokens=None):
    """Random lists with tfs 1..3 and positions 0, 2, 4, ...; fn_ids None: a field without a fieldnorm file."""
    table = O.fieldnorm_table()
    postings, positions, tp = [], [], []
    for i, df in enumerate(dfs):
        docs = set(int(d) for d in forced[i]) if i < len(forced) else set()
        pool = rng.permutation(max_doc)
        for d in pool:
            if len(docs) >= df:
                break
            docs.add(int(d))
        docs = sorted(docs)
        tfs = rng.integers(1, 4, size=len(docs))
        postings.append([(d, int(tf)) for d, tf in zip(docs, tfs)])
        positions.append([[2 * j for j in range(int(tf))] for tf in tfs])
        tp.append({d: ps for d, ps in zip(docs, positions[-1])})
    values = None if fn_ids is None else [int(table[i]) for i in fn_ids]
    seg = O.build_segment(max_doc, postings, values, record_option=O.WITH_FREQS_AND_POSITIONS, positions=positions,
                          total_num_tokens=total_num_tokens)
    return seg, tp, values


@functools.lru_cache(maxsize=None)
def fixture_x():
    """6 000 docs, 3 fields.  Field 0: 16 random lists (doc freqs 1, exactly 128, 129 = a block and a one-doc tail, < 128,
    at and above max_doc / 128 = own bitmap, below it = probe pool / range directory), fieldnorm ids 1..39 at random.
    Field 1: phrase_model's T2 (fieldnorms 20 / 40; tfs 254 / 255 / 256 / 300 at every slot of a group of four: the
    saturated tf byte reads packed values at a non-zero idx base; position runs across block edges at a non-zero pos
    base).  Field 2: two lists, no fieldnorm file (the constant id 1)."""
    rng = np.random.default_rng(20261019)
    t2 = PM.corpus("T2")
    md = t2.max_doc
    assert md == 6000
    ids0 = rng.integers(1, 40, size=md)
    seg0, tp0, val0 = _random_field(rng, md, X_DFS0, ids0)
    seg2, tp2, _ = _random_field(rng, md, [900, 2500], None, total_num_tokens=3 * md)
    assert seg2.fieldnorm is None
    return Fixture("X", [seg0, t2.segment(), seg2], [tp0, t2.tp, tp2], [val0, list(t2.fieldnorms), [1] * md])


Y_EDGE_DOCS = [0, 31, 32, 65535, 65536, PM.D_MAX_DOC - 1]
Y_DFS1 = [20000, 5000, 800, 300, 50, 3]


@functools.lru_cache(maxsize=None)
def fixture_y():
    """70 000 docs, 2 fields: the doc count crosses the 65 536-doc scoring tile and several tree tiles, the last bitmap
    word is partial.  Field 0: phrase_model's D (every fieldnorm 40).  Field 1: random lists under fieldnorm ids 1..39 at
    random, the first of them dense, every one of the first three with docs at 0, 31, 32, 65535, 65536 and max_doc - 1."""
    rng = np.random.default_rng(20261020)
    d = PM.corpus("D")
    md = d.max_doc
    assert md == 70_000 and md % 32 != 0
    ids1 = rng.integers(1, 40, size=md)
    seg1, tp1, val1 = _random_field(rng, md, Y_DFS1, ids1, forced=[Y_EDGE_DOCS] * 3)
    return Fixture("Y", [d.segment(), seg1], [d.tp, tp1], [list(d.fieldnorms), val1])


FIXTURES = {"X": fixture_x, "Y": fixture_y}


def flat_cases(fx):
    """Case 2 of the issue: single-term and flat queries of each non-primary field and of mixed fields, as
    tests/test_gpu_all.check_cases takes them: [(clauses, minimum_number_should_match)].  a = field 0, b = field 1, c = the
    last field (X: the one without a fieldnorm file)."""
    g = fx.gid
    last = len(fx.fields) - 1
    by_df = lambda f: sorted(range(len(fx.fields[f].terms)), key=lambda t: fx.fields[f].terms[t].doc_freq)  # noqa: E731
    a = by_df(0)
    b = by_df(1)
    ax, ay = g(0, a[-1]), g(0, a[-3])
    bx, by, bz = g(1, b[-1]), g(1, b[-2]), g(1, b[0])
    cz = g(last, by_df(last)[-1 if last != 1 else -3])
    T = lambda t: ("term", t)  # noqa: E731
    return [
        ([(S, T(bx))], 0),                                                                   # b:x
        ([(S, T(bz))], 0),                                                                   # b:z, the field's rarest list
        ([(S, T(cz))], 0),                                                                   # c:z
        ([(M, T(ax)), (M, T(by))], 0),                                                       # +a:x +b:y
        ([(S, T(ax)), (S, T(by)), (S, T(cz))], 0),                                           # a:x b:y c:z
        ([(S, ("union", [ax, bx])), (S, ("union", [ay, by]))], 0),                           # (a:x b:x) (a:y b:y)
        ([(M, ("union", [ax, bx])), (M, ("union", [ay, by]))], 0),                           # +(a:x b:x) +(a:y b:y)
        ([(S, ("union", [ax, bx])), (S, ("union", [ay, by])), (N, T(cz))], 0),               # ... -c:z
        ([(M, ("union", [ax, bx])), (M, ("union", [ay, by])), (N, T(cz))], 0),
        ([(S, T(ax)), (S, T(by)), (S, T(cz))], 2),                                           # at least 2 of clauses of three fields
        ([(M, T(by)), (S, T(ay))], 0),                                                       # +b:y a:y
    ]


def tree_cases(fx):
    """Case 3: nested shapes and phrase atoms with a field != 0, in tests/tree_shapes.py's spec form over global ids.  The
    phrase terms are phrase_model's terms 0 / 1 of the phrase field (X: field 1; Y: field 0 holds D, so the phrase atoms of
    Y are of the primary field and the nested terms of field 1)."""
    g = fx.gid
    pf = 1 if fx.name == "X" else 0   # the field with phrase_model positions
    of = 0 if fx.name == "X" else 1   # the other field
    by_df = sorted(range(len(fx.fields[of].terms)), key=lambda t: fx.fields[of].terms[t].doc_freq)
    ax = g(of, by_df[-1])
    by_, bz = g(pf, 5), g(pf, 6)
    p, q = g(pf, 0), g(pf, 1)
    return [
        ([(M, ax), (M, [(M, by_), (M, bz)], 0)], 0),          # +a:x +(+b:y +b:z)
        ([(S, [(M, by_), (M, bz)], 0), (S, ax)], 0),          # (+b:y +b:z) a:x
        ([(M, ax), (M, ("ph", [p, q]))], 0),                  # +a:x +"b:p b:q"
        ([(S, ("ph", [p, q])), (S, ax)], 0),                  # "b:p b:q" a:x
    ]


def set_members(fx):
    """Case 4: a term set with members of two fields (fixture X: fields 0 and 1)."""
    return [fx.gid(0, 8), fx.gid(1, 2)]


def add_set(L, key, members, weight):
    """A term set in the model's lists under `key` (the device's handle, or any hashable stand-in): present = the OR of its
    members' docs, score = the weight as given (ConstScorer: no norm, whatever the members' fields)."""
    present = np.zeros(L.fx.max_doc, bool)
    for g in members:
        L.need(g)
        present |= L.lists[g][0]
    L.lists[key] = (present, np.full(L.fx.max_doc, F32(weight), F32))
    L.weights[key] = float(F32(weight))
    return key


def set_cases(fx, s1, s25):
    """... beside a term of a third field (c:z, the field without a fieldnorm file): s1 / s25 = the keys of the set under
    weights 1.0 and 2.5."""
    cz = fx.gid(2, 1)
    T = lambda t: ("term", t)  # noqa: E731
    return [([(M, T(cz)), (M, T(s1))], 0), ([(S, T(cz)), (S, T(s25))], 0), ([(M, T(cz)), (N, T(s1))], 0),
            ([(M, T(s25)), (S, T(cz)), (S, T(fx.gid(1, 7)))], 0)]


PHRASE_QUERIES = ["p2", "p3", "rev2", "aa", "off02", "nomatch", "absent"]
