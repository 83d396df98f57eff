"""A literal model of BooleanWeight::complex_scorer (src/query/boolean_query/boolean_weight.rs:236-431) over dense numpy
arrays, for queries with AllQuery clauses: what tests/test_all_query_cpu.py checks tq_all_query_form against and what
tests/test_gpu_all.py takes its expectations from.  A scorer is (kind, present[bool n], score[f32 n]); every step below
names the lines it restates.  Nothing here comes from the product.

Clauses are (occur, what): what = ("all", boost) | ("absent",) | ("term", key) with key into `lists`, a dict
key -> (present, score) dense arrays; a ("union", [keys]) clause is a nested all-Should BooleanQuery of terms."""
import numpy as np

SHOULD, MUST, MUST_NOT = 0, 1, 2
ALL_EMPTY, ALL_PLAIN, ALL_BASED = 0, 1, 2
F = np.float32


class Scorer:
    def __init__(self, kind, present, score, cost=None, key=None):
        self.kind, self.present, self.score, self.key = kind, present, score, key
        self.cost = int(present.sum()) if cost is None else cost


def all_scorer(n):  # AllScorer: every doc, score 1.0 (all_query.rs:45-112)
    return Scorer("All", np.ones(n, bool), np.ones(n, F), cost=n)


def empty_scorer(n):
    return Scorer("Empty", np.zeros(n, bool), np.zeros(n, F), cost=0)


def sub_scorer(n, what, lists):
    """Weight::scorer of one clause."""
    if what[0] == "all":  # AllWeight::scorer (all_query.rs:24-31): a bare AllScorer at boost 1.0, else BoostScorer(AllScorer)
        if F(what[1]) == F(1.0):
            return all_scorer(n)
        return Scorer("Other", np.ones(n, bool), np.full(n, F(what[1]), F), cost=n)
    if what[0] == "absent":  # TermWeight::scorer without a TermInfo: EmptyScorer
        return empty_scorer(n)
    if what[0] == "union":  # a nested BooleanQuery of Should terms: BufferedUnionScorer / the one term itself
        subs = [sub_scorer(n, ("term", k), lists) for k in what[1] if k in lists]
        if not subs:
            return empty_scorer(n)
        if len(subs) == 1:
            return subs[0]
        return union(subs, n)
    p, s = lists[what[1]]
    return Scorer("Term", np.asarray(p, bool), np.where(p, np.asarray(s, F), F(0)).astype(F), key=what[1])


def union(scorers, n):
    """BufferedUnionScorer with the SumCombiner: 0 + the present scorers in order (buffered_union.rs, score_combiner.rs)."""
    present = np.zeros(n, bool)
    score = np.zeros(n, F)
    for sc in scorers:
        present |= sc.present
        score = np.where(sc.present, (score + sc.score).astype(F), score).astype(F)
    return Scorer("Other", present, score, cost=sum(sc.cost for sc in scorers))


def disjunction(scorers, n, need):
    """Disjunction (disjunction.rs:113-139): the docs at least `need` scorers hold; the present ones summed."""
    u = union(scorers, n)
    cnt = np.zeros(n, np.int32)
    for sc in scorers:
        cnt += sc.present
    keep = cnt >= need
    return Scorer("Other", keep, np.where(keep, u.score, F(0)).astype(F), cost=u.cost)


def intersect_scorers(scorers, n):
    """intersect_scorers (intersection.rs:20-56): one scorer is itself; else sorted by cost (stable), and
    Intersection::score = left + right + sum(others) (intersection.rs:325-329)."""
    if len(scorers) == 1:
        return scorers[0]
    order = sorted(range(len(scorers)), key=lambda i: scorers[i].cost)
    ss = [scorers[i] for i in order]
    present = np.ones(n, bool)
    for sc in ss:
        present &= sc.present
    score = (ss[0].score + ss[1].score).astype(F)
    if len(ss) > 2:
        others = np.zeros(n, F)
        for sc in ss[2:]:
            others = (others + sc.score).astype(F)
        score = (score + others).astype(F)
    return Scorer("Other", present, np.where(present, score, F(0)).astype(F), cost=ss[0].cost)


def remove_and_count_all_and_empty_scorers(scorers):  # boolean_weight.rs:440-456
    kept = [s for s in scorers if s.kind not in ("All", "Empty")]
    return kept, sum(s.kind == "All" for s in scorers), sum(s.kind == "Empty" for s in scorers)


def scorer_union(scorers, n):  # boolean_weight.rs:44-86: one scorer is itself, else the buffered union
    return scorers[0] if len(scorers) == 1 else union(scorers, n)


def effective_must_scorer(must, removed_all, n, trace):  # boolean_weight.rs:118-135
    if not must:
        if removed_all > 0:
            trace["all_back"] = True
            return all_scorer(n)
        return None
    return intersect_scorers(must, n)


def complex_scorer(clauses, minimum, lists, n):
    """-> (scorer, trace).  trace: empty (an EmptyScorer was returned), all_back (an AllScorer was put back in:
    effective_must_scorer / effective_should_scorer_for_union), eff_min (effective_minimum_number_should_match), kept
    (the positions of the clauses whose scorers were not removed)."""
    trace = {"empty": False, "all_back": False, "eff_min": 0, "kept": []}
    per = {SHOULD: [], MUST: [], MUST_NOT: []}
    for pos, (occur, what) in enumerate(clauses):  # per_occur_scorers, :220-234
        sc = sub_scorer(n, what, lists)
        sc.pos = pos
        per[occur].append(sc)

    def give_up():
        trace["empty"] = True
        return empty_scorer(n), trace

    must, must_all, must_empty = remove_and_count_all_and_empty_scorers(per[MUST])  # :246-248
    if must_empty > 0:  # :250-252
        return give_up()
    should, should_all, _ = remove_and_count_all_and_empty_scorers(per[SHOULD])  # :254-256
    exclude, exclude_all, _ = remove_and_count_all_and_empty_scorers(per[MUST_NOT])  # :258-262
    if exclude_all > 0:  # :264-267
        return give_up()
    eff_min = max(0, minimum - should_all)  # :269-271
    trace["eff_min"] = eff_min
    trace["kept"] = [s.pos for s in must + should + exclude]
    num_should = len(should)
    if eff_min > num_should:  # :275-279
        return give_up()
    if eff_min == 0 and num_should == 0:  # :281
        how, should_scorer = "ignored", None
    elif eff_min == 0:  # :282-286
        how, should_scorer = "optional", scorer_union(should, n)
    elif eff_min == 1:  # :287-291
        how, should_scorer = "required", scorer_union(should, n)
    elif eff_min == num_should:  # :292-297: no different from must clauses
        must = must + should
        how, should_scorer = "ignored", None
    else:  # :298-304
        how, should_scorer = "required", disjunction(should, n, eff_min)

    if how == "ignored":  # :309-351
        include = effective_must_scorer(must, must_all + should_all, n, trace)
        if include is None:
            return give_up()
    elif how == "optional":  # :352-388
        m = effective_must_scorer(must, must_all, n, trace)
        if m is None:
            if should_all > 0:  # effective_should_scorer_for_union, :144-171 (scoring enabled)
                trace["all_back"] = True
                include = union([should_scorer, all_scorer(n)], n)
            else:
                include = should_scorer
        else:  # RequiredOptionalScorer: req + opt where opt holds the doc (reqopt_scorer.rs:85-98)
            score = np.where(should_scorer.present, (m.score + should_scorer.score).astype(F), m.score).astype(F)
            include = Scorer("Other", m.present.copy(), np.where(m.present, score, F(0)).astype(F), cost=m.cost)
    else:  # required, :389-412
        m = effective_must_scorer(must, must_all, n, trace)
        include = should_scorer if m is None else intersect_scorers([m, should_scorer], n)
    if exclude:  # Exclude, :414-430
        gone = np.zeros(n, bool)
        for sc in exclude:
            gone |= sc.present
        keep = include.present & ~gone
        include = Scorer("Other", keep, np.where(keep, include.score, F(0)).astype(F))
    return include, trace


def implied_form(clauses, trace):
    """(kind, base, min_should, keep_mask) the literal model implies for a flat query of one-entry clauses."""
    if trace["empty"]:
        return (ALL_EMPTY, 0.0, 0, 0)
    mask = 0
    for pos in trace["kept"]:
        mask |= 1 << pos
    if trace["all_back"]:
        return (ALL_BASED, 1.0, trace["eff_min"], mask)
    return (ALL_PLAIN, 0.0, trace["eff_min"], mask)


def eval_form(form, clauses, lists, n):
    """What the normal form says the query computes: -> (present, score)."""
    kind, base, min_should, mask = form
    if kind == ALL_EMPTY:
        return np.zeros(n, bool), np.zeros(n, F)
    kept = [c for i, c in enumerate(clauses) if (mask >> i) & 1]
    if kind == ALL_PLAIN:  # the entries of keep_mask as a query without All clauses, minimum = min_should
        sc, _ = complex_scorer(kept, min_should, lists, n)
        return sc.present, sc.score
    cnt = np.zeros(n, np.int32)
    s = np.zeros(n, F)
    gone = np.zeros(n, bool)
    for occur, what in kept:
        sc = sub_scorer(n, what, lists)
        if occur == MUST_NOT:
            gone |= sc.present
        else:  # (an ALL-BASED query keeps Should and MustNot lists only)
            cnt += sc.present
            s = np.where(sc.present, (s + sc.score).astype(F), s).astype(F)
    present = (cnt >= min_should) & ~gone
    return present, np.where(present, (s + F(base)).astype(F), F(0)).astype(F)


def expect(clauses, minimum, lists, n, alive=None):
    """Ascending (docs, scores) of the query by the literal model, deleted docs removed."""
    sc, _ = complex_scorer(clauses, minimum, lists, n)
    present = sc.present if alive is None else sc.present & alive
    docs = np.nonzero(present)[0].astype(np.uint32)
    return docs, sc.score[docs].astype(F)


def top_k(docs, scores, k):
    """(score desc, doc asc), the order of TopNHeap::into_sorted_vec."""
    order = np.lexsort((docs, -scores.astype(np.float64)))[:k]
    return scores[order], docs[order]
