"""Plateau corpora and their float64 model: segments whose scores come in a handful of CLASSES shared by hundreds
or thousands of docs, so that the k-th rank of a top-k falls inside a tie and only the doc order decides the row.

Every doc has the same fieldnorm, so a posting's score depends on (list, tf) alone.
  * periodic(): list t holds the docs r_t (mod p_t) for small primes p_t, tf 1 or 2 in plateaus of a few thousand
    docs; two rare random lists (129 docs: one block + 1, and 300 docs) and 40 filler lists of 400 docs that only
    take the doc-matrix columns away from the rare ones.  2- to 4-term queries.
  * equal_df(): ten random lists of exactly the same doc frequency, tf 1: every term gets the same idf, a doc's
    score is decided by HOW MANY of the query's scoring lists hold it, and the planners' "by weight descending" /
    "by doc freq ascending" orders are all ties.  4- to 8-term unions, boolean and nested shapes.
  * phrase_pair(): two lists whose planted positions give every matching doc a phrase count of 1.

The model is numpy over the Python posting lists: BM25 in float64 from (doc freq, number of docs, average
fieldnorm, fieldnorm, tf) by the formula of src/query/bm25.rs:52-69,158-193 (idf = ln(1 + (N - n + 0.5) / (n + 0.5)),
weight = idf * (1 + K1), norm = K1 * (1 - B + B * fieldnorm / average), score = weight * tf / (tf + norm)); match
sets by set arithmetic over the lists; a query's expected row = its matches by (score class descending, segment
ordinal, doc ascending) without the deleted docs, cut at k.  No oracle executor is involved: the oracle only
serializes the lists into a segment (Corpus.seg), and tests/test_plateau_model_cpu.py holds the model against it.

The premises a (query, k) pair must meet before its row is trusted — class gap, straddle, class size inside one
8 192-posting run of the leading list — are functions here and asserts in tests/test_plateau_model_cpu.py; the
batches tests/test_gpu_plateau_ties.py runs are defined here, so both files see the same ones."""
import functools
import itertools
import math
from collections import namedtuple

import numpy as np

from oracle import oracle as O
from tests import tree_shapes as T

K1, B = 1.2, 0.75
M, S, N = O.MUST, O.SHOULD, O.MUST_NOT
MIN_GAP = 1e-3      # distinct classes differ by at least this, relative: 100 x BASELINE's 1e-5 score tolerance
SAME = 1e-12        # float64 sums of one class in two orders differ by less than this, relative
RUN = 8192          # postings of a 64-block task
MAX_DOC = 49_152 + 77
FIELDNORM = 10      # (fieldnorm ids below 40 are the values themselves: the quantisation keeps it)


class Corpus:
    def __init__(self, name, max_doc, lists, positions=None):
        self.name, self.max_doc, self.lists, self.positions = name, int(max_doc), lists, positions
        self._seg = None
        self._tf = {}

    @property
    def seg(self):
        """The segment, through the oracle's serializers (built once)."""
        if self._seg is None:
            pl = [list(zip(d.tolist(), f.tolist())) for d, f in self.lists]
            opt = O.WITH_FREQS_AND_POSITIONS if self.positions is not None else O.WITH_FREQS
            self._seg = O.build_segment(self.max_doc, pl, [FIELDNORM] * self.max_doc, record_option=opt, positions=self.positions)
        return self._seg

    def df(self, t):
        return len(self.lists[t][0])

    def tf(self, t):
        """tf of list t per doc (0: the doc is not in it)"""
        if t not in self._tf:
            a = np.zeros(self.max_doc, np.int64)
            a[self.lists[t][0]] = self.lists[t][1]
            self._tf[t] = a
        return self._tf[t]

    def weight(self, dfs, copies=1, boost=1.0):
        """Bm25Weight.weight of a term (or, several doc freqs, of a phrase: idfs summed) over `copies` copies of the segment"""
        n = copies * self.max_doc
        return boost * (1.0 + K1) * sum(math.log(1.0 + (n - copies * df + 0.5) / (copies * df + 0.5)) for df in dfs)

    def term_scores(self, t, copies=1, boost=1.0):
        """float64 score of list t per doc (0.0: not in it).  The average fieldnorm IS the fieldnorm: norm = K1."""
        tf = self.tf(t).astype(np.float64)
        return self.weight([self.df(t)], copies, boost) * tf / (tf + K1 * (1.0 - B + B * FIELDNORM / FIELDNORM)) * (tf > 0)


def _periodic_lists():
    rng = np.random.default_rng(20261021)
    lists = []
    for p, r, plateau in ((2, 0, 8192), (3, 1, 4096), (5, 2, 6144), (7, 3, 5120), (11, 4, 7168)):
        docs = np.arange(r, MAX_DOC, p, dtype=np.int64)
        lists.append((docs, 1 + (docs // plateau) % 2))
    for df in [129, 300] + [400] * 40:  # 5, 6: the rare lists; 7..46: fillers (never queried)
        docs = np.sort(rng.choice(MAX_DOC, size=df, replace=False)).astype(np.int64)
        lists.append((docs, np.ones(df, np.int64)))
    return lists


@functools.lru_cache(None)
def periodic():
    return Corpus("periodic", MAX_DOC, _periodic_lists())


EQ_DF, EQ_LISTS = 9000, 10


@functools.lru_cache(None)
def equal_df():
    rng = np.random.default_rng(20261022)
    lists = []
    for _ in range(EQ_LISTS):
        docs = np.sort(rng.choice(MAX_DOC, size=EQ_DF, replace=False)).astype(np.int64)
        lists.append((docs, np.ones(EQ_DF, np.int64)))
    return Corpus("equal_df", MAX_DOC, lists)


PHRASE_MAX_DOC = 20_480 + 77


@functools.lru_cache(None)
def phrase_pair():
    """List 0 = the even docs, list 1 = the multiples of 3, tf 1 or 2.  In the docs 6 (mod 12) list 0 stands right
    before list 1 exactly once ("0 1" matches with a phrase count of 1: positions [4] or [4, 9] against [5] or [1, 5]);
    in the docs 0 (mod 12) it stands behind it: both lists hold the doc, the phrase does not."""
    d0 = np.arange(0, PHRASE_MAX_DOC, 2, dtype=np.int64)
    d1 = np.arange(0, PHRASE_MAX_DOC, 3, dtype=np.int64)
    t0, t1 = 1 + (d0 // 2048) % 2, 1 + (d1 // 3072) % 2
    p0 = [([4] if d % 12 else [7]) + ([9] if f == 2 else []) for d, f in zip(d0.tolist(), t0.tolist())]
    p1 = [([1] if f == 2 else []) + [5] for f in t1.tolist()]
    return Corpus("phrase_pair", PHRASE_MAX_DOC, [(d0, t0), (d1, t1)], positions=[p0, p1])


CORPORA = {"periodic": periodic, "equal_df": equal_df, "phrase_pair": phrase_pair}

# ---------------------------------------------------------------------------------------------------- queries
# kind: "and" / "or" (spec = (terms, boosts | None)), "bool" (spec = (terms, occurs, clause_of | None, msm)),
# "tree" (spec = (clause list of tests/tree_shapes.py, top-level msm)), "phrase" (spec = terms)
Q = namedtuple("Q", "kind spec")


def q_and(terms, boosts=None):
    return Q("and", (tuple(terms), None if boosts is None else tuple(boosts)))


def q_or(terms, boosts=None):
    return Q("or", (tuple(terms), None if boosts is None else tuple(boosts)))


def q_bool(terms, occurs, clause_of=None, msm=0):
    return Q("bool", (tuple(terms), tuple(occurs), None if clause_of is None else tuple(clause_of), msm))


def q_tree(shape, terms):
    build, msm = shape
    return Q("tree", (build(list(terms)), msm))


def q_phrase(terms):
    return Q("phrase", tuple(terms))


def to_device(ta, q):
    """The tuple DeviceIndex.search takes."""
    if q.kind in ("and", "or"):
        terms, boosts = q.spec
        head = (O.MODE_AND if q.kind == "and" else O.MODE_OR, list(terms))
        return head if boosts is None else head + ({"boosts": list(boosts)},)
    if q.kind == "bool":
        terms, occ, cof, msm = q.spec
        return (ta.MODE_BOOL, list(terms), list(occ), None if cof is None else list(cof), msm)
    if q.kind == "tree":
        return T.to_device(ta, q.spec[0], q.spec[1])
    return (O.MODE_PHRASE, list(q.spec))


def _combine(md, items, msm):
    """A BooleanQuery over evaluated clauses, items = [(occur, match bool[md], score f64[md])]: every Must clause
    matches; with a Must clause the Should clauses are optional unless `msm` asks for some, without one at least
    max(1, msm) of them match; no MustNot clause matches; MustNot clauses alone match nothing.  Score = the sum of
    the matching Must and Should clauses' scores."""
    must = [x for x in items if x[0] == M]
    should = [x for x in items if x[0] == S]
    if not must and not should:
        return np.zeros(md, bool), np.zeros(md)
    match = np.ones(md, bool)
    score = np.zeros(md)
    n_hit = np.zeros(md, np.int64)
    for _, hit, sc in must:
        match &= hit
        score = score + sc
    for _, hit, sc in should:
        n_hit += hit
        score = score + np.where(hit, sc, 0.0)
    need = msm if must else max(1, msm)
    if need:
        match &= n_hit >= need
    for o, hit, _ in items:
        if o == N:
            match &= ~hit
    return match, np.where(match, score, 0.0)


def evaluate(corpus, q, copies=1):
    """(match bool[max_doc], score f64[max_doc]) of the query in ONE copy of the segment, under the statistics of
    `copies` identical segments."""
    md = corpus.max_doc

    def leaf(t, boost=1.0):
        return corpus.tf(t) > 0, corpus.term_scores(t, copies, boost)

    if q.kind in ("and", "or"):
        terms, boosts = q.spec
        occ = M if q.kind == "and" else S
        return _combine(md, [(occ,) + leaf(t, 1.0 if boosts is None else boosts[i]) for i, t in enumerate(terms)], 0)
    if q.kind == "bool":
        terms, occs, cof, msm = q.spec
        cof = list(range(len(terms))) if cof is None else cof
        items = []
        for c in sorted(set(cof)):  # a clause of several terms is their union
            members = [i for i in range(len(terms)) if cof[i] == c]
            items.append((occs[members[0]],) + _combine(md, [(S,) + leaf(terms[i]) for i in members], 0))
        return _combine(md, items, msm)
    if q.kind == "tree":
        spec, msm = q.spec

        def member(m):
            if isinstance(m, tuple) and m[0] == "any":
                return _combine(md, [(S,) + leaf(t) for t in m[1]], 0)
            if isinstance(m, (list, tuple)):
                return _combine(md, [(M,) + leaf(t) for t in m], 0)
            return leaf(m)

        items = []
        for cl in spec:
            if isinstance(cl[1], list):
                items.append((cl[0],) + _combine(md, [(o,) + member(m) for o, m in cl[1]], cl[2] if len(cl) > 2 else 0))
            else:
                items.append((cl[0],) + member(cl[1]))
        return _combine(md, items, msm)
    # phrase of two terms: the docs where a position of the first stands right before one of the second, scored
    # with the summed idfs and the number of such places as tf
    a, b = q.spec
    count = np.zeros(md, np.float64)
    pos_b = dict(zip(corpus.lists[b][0].tolist(), corpus.positions[b]))
    for d, pa in zip(corpus.lists[a][0].tolist(), corpus.positions[a]):
        if d in pos_b:
            count[d] = sum(1 for p in pa if p + 1 in pos_b[d])
    w = corpus.weight([corpus.df(a), corpus.df(b)], copies)
    return count > 0, w * count / (count + K1) * (count > 0)


Answer = namedtuple("Answer", "docs scores cls n_classes min_gap")  # docs ascending; cls 0 = the best class


def answer(corpus, q, deleted=(), copies=1):
    """The query's alive matches, their float64 scores and score classes."""
    match, score = evaluate(corpus, q, copies)
    if len(deleted):
        match = match.copy()
        match[np.asarray(deleted, np.int64)] = False
    docs = np.nonzero(match)[0]
    sc = score[docs]
    uniq = np.unique(sc)[::-1]  # descending
    gaps = (uniq[:-1] - uniq[1:]) / uniq[:-1] if len(uniq) > 1 else np.zeros(0)
    new_class = np.concatenate([[True], gaps >= SAME]) if len(uniq) else np.zeros(0, bool)
    cls_of_uniq = np.cumsum(new_class) - 1
    real = gaps[gaps >= SAME]
    cls = cls_of_uniq[np.searchsorted(-uniq, -sc)] if len(uniq) else np.zeros(0, np.int64)
    return Answer(docs, sc, cls, int(new_class.sum()), float(real.min()) if len(real) else float("inf"))


def row(ans, k, copies=1):
    """The expected top-k: [(segment ordinal, doc, float64 score)] by (class, segment ordinal, doc ascending)."""
    n = len(ans.docs)
    ords = np.repeat(np.arange(copies), n)
    docs, cls, sc = np.tile(ans.docs, copies), np.tile(ans.cls, copies), np.tile(ans.scores, copies)
    order = np.lexsort((docs, ords, cls))[:k]
    return [(int(ords[i]), int(docs[i]), float(sc[i])) for i in order]


def kth_class(ans, k, copies=1):
    """(above, tied, class index) of rank k: docs in better classes, docs in the k-th rank's class (over all copies);
    None if the query has fewer than k matches."""
    if copies * len(ans.docs) < k:
        return None
    counts = np.bincount(ans.cls, minlength=ans.n_classes) * copies
    above = 0
    for c, n in enumerate(counts.tolist()):
        if above + n >= k:
            return above, n, c
        above += n
    raise AssertionError("unreachable")


def straddles(ans, k, copies=1):
    """The k-th rank cuts a class in two: docs of one score on both sides of the cut."""
    kc = kth_class(ans, k, copies)
    return kc is not None and kc[0] < k < kc[0] + kc[1]


def leading_list(corpus, q):
    """The list whose postings drive the query in the shared launches: the rarest required list (intersections, by
    doc freq, stable), else the rarest = highest-weight optional one."""
    if q.kind in ("and", "or"):
        terms = q.spec[0]
    elif q.kind == "bool":
        terms = [t for t, o in zip(q.spec[0], q.spec[1]) if o == M] or [t for t, o in zip(q.spec[0], q.spec[1]) if o == S]
    else:
        raise ValueError(q.kind)
    return min(terms, key=corpus.df)


def kth_class_in_one_run(corpus, q, ans, k):
    """The most docs of the k-th rank's class that lie inside one run of RUN postings of the query's leading list."""
    kc = kth_class(ans, k)
    if kc is None:
        return 0
    lead = corpus.lists[leading_list(corpus, q)][0]
    docs = ans.docs[ans.cls == kc[2]]
    at = np.searchsorted(lead, docs)
    at = at[(at < len(lead)) & (lead[np.minimum(at, len(lead) - 1)] == docs)]
    return int(np.bincount(at // RUN).max()) if len(at) else 0


# ---------------------------------------------------------------------------------------------------- batches
Batch = namedtuple("Batch", "name corpus queries ks deleted shared copies")


def _usable(corpus, queries, deleted=(), copies=1):
    """Queries whose distinct classes differ by at least MIN_GAP (the others are not used at all)."""
    return [q for q in queries if answer(corpus, q, deleted, copies).min_gap >= MIN_GAP]


BOOSTS2 = [(1.0, 1.0), (2.0, 1.0), (1.0, 1.5), (0.5, 3.0), (1.25, 0.75), (3.0, 2.0), (1.0, 4.0), (2.5, 0.5)]


def _per_query_ands():
    c = periodic()
    qs = [q_and(p) for p in ([0, 1], [1, 0], [1, 2], [0, 4], [2, 3], [0, 1, 2], [1, 2, 3], [0, 1, 2, 3], [5, 0], [6, 1], [5, 6])]
    return Batch("per_query_ands", "periodic", _usable(c, qs), (1, 64, 65, 100), (), False, 1)


def _shared_ands():
    """2-term ANDs over the periodic lists under fifteen boost pairs (distinct weights: distinct queries for the
    planner's dedupe), 36 more variants of [0, 1] (its leader, list 1, then leads more than 32 distinct queries: two
    groups), 3- and 4-term ANDs, and the first 30 queries once more (twins)."""
    c = periodic()
    qs = [q_and(p, b) for p in itertools.combinations(range(5), 2) for b in BOOSTS2 + [(y, x) for x, y in BOOSTS2[1:]]]
    qs += [q_and([0, 1], (1.0 + 0.125 * i, 1.0 + 0.0625 * (i % 7))) for i in range(1, 37)]
    qs += [q_and(p, b) for p in itertools.combinations(range(5), 3) for b in (None, (1.0, 2.0, 1.5))]
    qs += [q_and(p) for p in itertools.combinations(range(5), 4)]
    qs = _usable(c, qs)
    return Batch("shared_ands", "periodic", qs + qs[:30], (1, 16, 17, 64, 100), (), True, 1)


BOOL_SHAPES = [([M, S, N], None, 0),               # +a b -c
               ([M, M, M], [0, 1, 1], 0),          # +a +(b OR c)
               ([M, M, M, M], [0, 0, 1, 1], 0),    # +(a OR b) +(c OR d)
               ([M, S, S], None, 1), ([S, S, S], None, 2), ([M, S, S, S], None, 2)]  # minimum_number_should_match


def _shared_bools():
    """The boolean shapes over the equal-df lists, each over four choices of lists.  Deleted: the four lowest docs of
    the class each (query, k) cuts — the cut then falls on the next ones."""
    c = equal_df()
    rng = np.random.default_rng(7)
    qs = []
    for occ, cof, msm in BOOL_SHAPES * 4:
        qs.append(q_bool(rng.choice(EQ_LISTS, size=len(occ), replace=False).tolist(), occ, cof, msm))
    qs = _usable(c, qs)
    ks = (1, 10, 17, 100)
    deleted = set()
    for q in qs:
        a = answer(c, q)
        for k in ks:
            kc = kth_class(a, k)
            if kc is not None:
                deleted.update(a.docs[a.cls == kc[2]][:4].tolist())
    return Batch("shared_bools", "equal_df", _usable(c, qs, tuple(sorted(deleted))), ks, tuple(sorted(deleted)), True, 1)


def _shared_unions_periodic():
    """2- to 4-term unions over the periodic lists, with list 5 (no bitmap at dense_ratio 200) and list 6 (a bitmap
    but, behind the 40 fillers, no doc-matrix column: its signature bit)."""
    c = periodic()
    qs = [q_or(p, b) for p in ([0, 1], [1, 2], [0, 2]) for b in BOOSTS2[:4]]
    qs += [q_or(p) for p in ([0, 1, 2], [1, 2, 3], [0, 1, 5], [0, 1, 6], [1, 5, 6], [0, 2, 6], [5, 6], [2, 3, 4], [0, 1, 2, 5], [1], [4])]
    return Batch("shared_unions_periodic", "periodic", _usable(c, qs), (1, 16, 17, 64, 128), (), True, 1)


def _shared_unions_equal_df():
    c = equal_df()
    rng = np.random.default_rng(11)
    qs = [q_or(rng.choice(EQ_LISTS, size=n, replace=False).tolist()) for n in (4, 5, 6, 7, 8, 2, 3) for _ in range(4)]
    return Batch("shared_unions_equal_df", "equal_df", _usable(c, qs), (1, 16, 17, 64, 128), (), True, 1)


def _per_query_unions():
    c = periodic()
    qs = [q_or(p) for p in ([0, 1], [1, 2], [0, 1, 2], [0, 1, 5], [2, 3, 4], [5, 6], [3])]
    return Batch("per_query_unions", "periodic", _usable(c, qs), (10, 128, 129, 300), (), False, 1)


def _per_query_unions_equal_df():
    c = equal_df()
    qs = [q_or(list(range(n))) for n in (2, 4, 5, 8)] + [q_or([9, 3, 7, 1, 5])]
    return Batch("per_query_unions_equal_df", "equal_df", _usable(c, qs), (10, 128, 129, 300), (), False, 1)


TREE_SHAPES = [T.SHAPES[0], T.SHAPES[4], T.SHAPES[8]]  # +a +((+b +c) d);  +a +(b c d)~2;  (+a +b) (+c +d) (+e +f +g)


def _trees():
    c = equal_df()
    rng = np.random.default_rng(13)
    qs = [q_tree(sh, rng.choice(EQ_LISTS, size=8, replace=False).tolist()) for sh in TREE_SHAPES for _ in range(3)]
    return Batch("trees", "equal_df", _usable(c, qs), (10, 100), (), False, 1)


def _phrases():
    return Batch("phrases", "phrase_pair", [q_phrase([0, 1])], (10,), (), False, 1)


def _two_segment_ands():
    c = periodic()
    qs = [q_and(p, b) for p in itertools.combinations(range(5), 2) for b in BOOSTS2[:3]]
    qs += [q_and(p) for p in ([0, 1, 2], [0, 1, 2, 3], [0, 2, 3, 4], [1, 2, 3, 4])]
    return Batch("two_segment_ands", "periodic", _usable(c, qs, (), 2), (10,), (), True, 2)


def _two_segment_unions():
    c = periodic()
    qs = [q_or(p, b) for p in ([0, 1], [1, 2], [0, 2]) for b in BOOSTS2[:3]]
    qs += [q_or(p) for p in ([0, 1, 2], [0, 1, 5], [5, 6], [1])]
    return Batch("two_segment_unions", "periodic", _usable(c, qs, (), 2), (10,), (), True, 2)


_BUILDERS = {b.__name__[1:]: b for b in (_per_query_ands, _shared_ands, _shared_bools, _shared_unions_periodic, _shared_unions_equal_df,
                                         _per_query_unions, _per_query_unions_equal_df, _trees, _phrases, _two_segment_ands,
                                         _two_segment_unions)}
BATCH_NAMES = tuple(_BUILDERS)


@functools.lru_cache(None)
def batch(name):
    return _BUILDERS[name]()


@functools.lru_cache(None)
def answers(name):
    """[Answer] of the batch's queries (shared by the tests: computed once, never modified)."""
    b = batch(name)
    c = CORPORA[b.corpus]()
    return [answer(c, q, b.deleted, b.copies) for q in b.queries]
