"""A plain model of exact-phrase matching (PhraseScorer, src/query/phrase_query/phrase_scorer.rs:82-136,347-507) and the
corpora of tests/test_phrase_model_cpu.py and tests/test_gpu_phrase_positions.py.

The model works from TOKEN-LEVEL input — per term {doc: [positions]}, non-decreasing, repeats allowed (the reference's
NgramTokenizer writes position 0 on every token, synonym filters repeat positions) — never from encoded bytes, and the
functions of part 1 call neither the oracle nor the library.

  adjusted position = position + max(offsets) - offsets[m]                               (phrase_scorer.rs:372-385)
  phrase count      = sum over values v of min over terms m of multiplicity_m(v)         (intersection / intersection_count)
  score             = (1 + K1) * sum idf * c / (c + K1 * (1 - B + B * dl / avgdl)),      idf = ln(1 + (N - n + .5) / (n + .5))

phrase_counts_merge restates the reference's sequential two-pointer merges literally; the CPU test asserts that both give
the same counts on every corpus, which is the proof that the multiset formula is the reference's semantics whatever the
order of the terms."""
import bisect
import collections
import functools
import math

import numpy as np

K1, B = 1.2, 0.75
ABSENT = 99  # a term id no corpus has


# ------------------------------------------------------------------------------------------------ 1. the model
def _lists(term_positions, t):
    return term_positions[t] if 0 <= t < len(term_positions) else {}


def _candidates(term_positions, terms, alive):
    docs = None
    for t in terms:
        ks = set(_lists(term_positions, t))
        docs = ks if docs is None else docs & ks
    docs = sorted(docs or ())
    return [d for d in docs if alive is None or alive[d]]


def and_docs(term_positions, terms, alive=None):
    """The docs that hold every term of the phrase (its candidates), ascending."""
    return _candidates(term_positions, terms, alive)


def near_misses(term_positions, terms, offsets, alive=None):
    """The candidates without a match in which the SECOND term stands exactly one position late somewhere."""
    counts = phrase_counts(term_positions, terms, offsets, alive)
    out = []
    for d in _candidates(term_positions, terms, alive):
        if d in counts:
            continue
        first = {p - offsets[0] for p in term_positions[terms[0]][d]}
        if any(p - offsets[1] - 1 in first for p in term_positions[terms[1]][d]):
            out.append(d)
    return out


def phrase_counts(term_positions, terms, offsets, alive=None):
    """{doc: phrase count} of the docs with a count >= 1."""
    top = max(offsets)
    out = {}
    for d in _candidates(term_positions, terms, alive):
        total = None
        for t, o in zip(terms, offsets):
            c = collections.Counter(p + top - o for p in term_positions[t][d])
            total = c if total is None else total & c  # (& of Counters: the minimum multiplicity per value)
        n = sum(total.values())
        if n:
            out[d] = n
    return out


def _intersection(left, right):  # phrase_scorer.rs:111-136
    li = ri = 0
    out = []
    while li < len(left) and ri < len(right):
        if left[li] < right[ri]:
            li += 1
        elif left[li] == right[ri]:
            out.append(left[li])
            li += 1
            ri += 1
        else:
            ri += 1
    return out


def _intersection_count(left, right):  # phrase_scorer.rs:82-104
    li = ri = count = 0
    while li < len(left) and ri < len(right):
        if left[li] < right[ri]:
            li += 1
        elif left[li] == right[ri]:
            count += 1
            li += 1
            ri += 1
        else:
            ri += 1
    return count


def phrase_counts_merge(term_positions, terms, offsets, alive=None):
    """The same counts by the reference's own steps: `left` = the first term's adjusted positions, intersected in place
    with every term but the last (compute_phrase_match), then intersection_count against the last."""
    top = max(offsets)
    out = {}
    for d in _candidates(term_positions, terms, alive):
        adj = [[p + top - o for p in term_positions[t][d]] for t, o in zip(terms, offsets)]
        left = adj[0]
        for right in adj[1:-1]:
            left = _intersection(left, right)
        n = _intersection_count(left, adj[-1])
        if n:
            out[d] = n
    return out


def bm25(weight, count, dl, avgdl):
    return weight * count / (count + K1 * (1.0 - B + B * dl / avgdl))


def phrase_weight(term_positions, terms, max_doc):
    idf = 0.0
    for t in terms:  # (a repeated term counts once per occurrence: Bm25Weight::for_terms over the phrase's terms)
        n = len(_lists(term_positions, t))
        idf += math.log(1.0 + (max_doc - n + 0.5) / (n + 0.5))
    return (1.0 + K1) * idf


def phrase_scores(term_positions, terms, offsets, fieldnorms, alive=None):
    """(docs ascending uint32, float64 scores, counts) from the definition."""
    max_doc = len(fieldnorms)
    counts = phrase_counts(term_positions, terms, offsets, alive)
    avgdl = float(sum(int(f) for f in fieldnorms)) / max_doc
    w = phrase_weight(term_positions, terms, max_doc)
    docs = np.array(sorted(counts), np.uint32)
    cs = np.array([counts[int(d)] for d in docs], np.int64)
    sc = np.array([bm25(w, counts[int(d)], float(fieldnorms[int(d)]), avgdl) for d in docs], np.float64)
    return docs, sc, cs


def top_k(docs, scores, k):
    """(score desc, doc asc), the order of TopNHeap::into_sorted_vec (as tests/all_model.py)."""
    order = np.lexsort((docs, -np.asarray(scores, np.float64)))[:k]
    return np.asarray(scores)[order], np.asarray(docs)[order]


def min_relative_gap(weight, counts, dl, avgdl):
    """The smallest relative distance between score(c) and score(c + 1) over the counts given."""
    gap = 1.0
    for c in counts:
        a, b = bm25(weight, c, dl, avgdl), bm25(weight, c + 1, dl, avgdl)
        gap = min(gap, (b - a) / b)
    return gap


# ------------------------------------------------------------------------------------------------ 2. the corpora
NT = 8  # terms 0..7 of every corpus, by construction in ascending doc freq except where a corpus says otherwise
QUERIES = [  # (name, term ids, offsets)
    ("p2", [0, 1], [0, 1]), ("p3", [0, 1, 2], [0, 1, 2]), ("p4", [0, 1, 2, 3], [0, 1, 2, 3]),
    ("p5", [0, 1, 2, 3, 4], [0, 1, 2, 3, 4]), ("p8", list(range(8)), list(range(8))),
    ("rev2", [1, 0], [0, 1]), ("rev4", [3, 2, 1, 0], [0, 1, 2, 3]),
    ("off02", [0, 2], [0, 2]), ("off013", [0, 1, 3], [0, 1, 3]),
    ("aa", [0, 0], [0, 1]), ("aba", [0, 1, 0], [0, 1, 2]),
    ("nomatch", [0, 1], [0, 100000]), ("absent", [0, ABSENT], [0, 1]),
]
MAIN = 0  # the query the per-corpus input conditions are stated for


class Corpus:
    def __init__(self, name, term_positions, fieldnorms, deleted=None, notes=None):
        self.name = name
        self.tp = term_positions
        self.fieldnorms = fieldnorms
        self.max_doc = len(fieldnorms)
        self.deleted = None if deleted is None else sorted(int(d) for d in deleted)
        self.alive = None
        if deleted is not None:
            self.alive = np.ones(self.max_doc, bool)
            self.alive[self.deleted] = False
        self.notes = notes or {}
        self.queries = QUERIES
        self._seg = None

    def dfs(self):
        return [len(t) for t in self.tp]

    def segment(self):
        """The corpus serialised through the oracle's PostingsSerializer / PositionSerializer."""
        if self._seg is None:
            from oracle import oracle as O

            postings = [[(d, len(t[d])) for d in sorted(t)] for t in self.tp]
            positions = [[t[d] for d in sorted(t)] for t in self.tp]
            self._seg = O.build_segment(self.max_doc, postings, self.fieldnorms, record_option=O.WITH_FREQS_AND_POSITIONS,
                                        positions=positions)
        return self._seg

    @functools.lru_cache(maxsize=None)
    def expect(self, qi):
        """(docs, float64 scores, counts) of query qi over the alive docs."""
        _, terms, offs = self.queries[qi]
        return phrase_scores(self.tp, terms, offs, self.fieldnorms, self.alive)


def _all_terms(reps, shift=lambda t: t):
    return {t: [x + shift(t) for x in reps] for t in range(NT)}


def _plant(tp, doc, per_term):
    for t, ps in per_term.items():
        assert list(ps) == sorted(ps) and len(ps) >= 1
        tp[t][doc] = list(ps)


def _background(rng, max_doc, dfs, pos_hi=30):
    tp = []
    for df in dfs:
        docs = np.sort(rng.choice(max_doc, size=df, replace=False))
        two = rng.random(df) < 0.25
        first = rng.integers(0, pos_hi, size=df)
        step = rng.integers(1, 9, size=df)
        tp.append({int(d): ([int(p), int(p + s)] if w else [int(p)]) for d, w, p, s in zip(docs, two, first, step)})
    return tp


def _plant_generic(tp, max_doc, taken):
    """What every corpus holds besides its own edges: 24 docs that hold the phrase 0 1 .. 7 (8 of them twice, 6 with
    term 0 on three consecutive positions: "a a" and "a b a"), 6 that hold it in reverse, and 24 near misses (every term,
    term 1 one position late)."""
    def free(d):
        while d in taken:
            d += 1
        assert d < max_doc
        taken.add(d)
        return d

    for i in range(24):
        d = free(100 + 37 * i)
        p = 3 + i % 11
        per = _all_terms([p, p + 10] if i % 3 == 0 else [p])
        if i % 4 == 1:
            per[0] = [p, p + 1, p + 2]
        _plant(tp, d, per)
    for i in range(6):
        _plant(tp, free(1500 + 53 * i), _all_terms([2 + i], shift=lambda t: 7 - t))
    for i in range(24):
        per = _all_terms([4 + i % 9])
        per[1] = [x + 1 for x in per[1]]
        _plant(tp, free(2000 + 41 * i), per)


# ---- P: the edges of the position stream
P_WIDTHS0 = [0, 1, 7, 8, 9, 16, 31, 32]     # bit widths of term 0's bitpacked position blocks
P_LEAD_IN1 = 512  # fillers in front of term 1's stream: clearly more postings than term 0, the same in-block indices
P_WIDTHS1 = [1] * 4 + [1, 1, 7, 8, 9, 16, 31, 32, 0]  # ... of term 1's (its width-0 block lies where term 0 is in its vint tail)


def build_P():
    """Terms 0 (leader of "0 1") and 1 are laid out delta by delta: filler docs (one position each, in that term only)
    bring the stream to the index where a matching doc's run is to start.  Per bitpacked block: a run inside it, and
    a run that ends at in-block index 127 (even blocks) or starts there and continues in the next block (odd blocks; the
    last one continues in the vint tail).  A block's width is that of its matching docs' first positions, 2^(w-1); width
    0 is all zero deltas: positions [0, 0].  Term 1's width-0 block matches "1 0".  Term 2 has < 128 positions (no
    bitpacked block), term 3 exactly 256 (no tail)."""
    tp = [dict() for _ in range(NT)]
    cur = [0, 0]
    nxt = [100]  # (docs 0..99: fillers of term 3, so that its matching docs straddle its block edge)
    widths = (P_WIDTHS0, P_WIDTHS1)

    def new_doc():
        nxt[0] += 1
        return nxt[0] - 1

    def fill(t, target):
        assert cur[t] <= target, (t, cur[t], target)
        while cur[t] < target:
            b = cur[t] >> 7
            tp[t][new_doc()] = [0 if b < len(widths[t]) and widths[t][b] == 0 else 1]
            cur[t] += 1

    def key(at0, at1, pos0, pos1):
        if at0 is not None:
            fill(0, at0)
        if at1 is not None:
            fill(1, at1 + P_LEAD_IN1)
        d = new_doc()
        per = _all_terms(pos0)
        per[0], per[1] = pos0, pos1
        _plant(tp, d, per)
        cur[0] += len(pos0)
        cur[1] += len(pos1)
        return d

    for d in range(100):
        tp[3][d] = [3]
    for b in range(8):
        base = 128 * b
        if b == 0:  # term 0: width 0
            key(base + 40, base + 40, [0, 0], [1])
            key(base + 43, base + 43, [0, 0], [1, 1])
            key(base + 126, base + 126, [0, 0], [1, 1])
        elif b == 1:  # width 1 on both sides
            key(base + 40, base + 40, [0], [1])
            key(base + 41, base + 41, [0, 1], [1, 2])
            key(base + 127, base + 127, [0, 1, 2], [1, 2, 3])
        else:
            p = 1 << (P_WIDTHS0[b] - 1)
            key(base + 40, base + 40, [p], [p + 1])
            key(base + 41, base + 41, [p, p + 5], [p + 1, p + 6])
            if b % 2 == 0:
                key(base + 126, base + 126, [p, p + 5], [p + 1, p + 6])
            elif b < 7:
                key(base + 127, base + 127, [p, p + 5, p + 10], [p + 1, p + 6, p + 11])
            else:  # term 0 continues in its tail, term 1 in its width-0 block: zero deltas
                key(base + 127, base + 127, [p, p + 5, p + 10], [p + 1, p + 1, p + 1])
    # term 1's width-0 block (indices 1024..1151), term 0 in its tail: matches of "1 0"
    key(None, 1024 + 10, [1], [0, 0])
    key(None, 1024 + 13, [1, 1], [0, 0])
    key(None, 1024 + 127, [1, 6, 11], [0, 5, 10])  # term 1: starts in its last bitpacked block, continues in the tail
    # wholly in the tail on both sides
    key(None, None, [7], [8])
    key(None, None, [7, 12], [8, 13])
    for i in range(3):  # the phrase in reverse
        _plant(tp, new_doc(), _all_terms([2 + i], shift=lambda t: 7 - t))
        cur[0] += 1
        cur[1] += 1
    for i in range(24):  # near misses
        d = new_doc()
        per = _all_terms([4 + i % 9])
        per[1] = [x + 1 for x in per[1]]
        _plant(tp, d, per)
        cur[0] += 1
        cur[1] += 1
    assert 1024 < cur[0] < 1152 and 1152 < cur[1] - P_LEAD_IN1 < 1280
    n2 = sum(len(p) for p in tp[2].values())
    n3 = sum(len(p) for p in tp[3].values())
    assert n2 < 128 and n3 < 256
    for _ in range(256 - n3):
        tp[3][new_doc()] = [3]
    for t, df in ((4, 300), (5, 350), (6, 400), (7, 450)):
        while len(tp[t]) < df:
            tp[t][new_doc()] = [1]
    max_doc = max(4500, nxt[0] + 1)
    return Corpus("P", tp, [40] * max_doc)


# ---- T: term freqs around the hand-over between the register path and the cursor merge, and around the saturated tf byte
T_DFS = [300, 700, 800, 900, 1000, 1100, 1200, 1300]
T_SMALL_TFS = [1, 2, 8, 9, 16, 40]
T_BIG_TFS = [254, 255, 256, 300]


def _build_T_positions():
    rng = np.random.default_rng(1801)
    max_doc = 6000
    tp = _background(rng, max_doc, T_DFS)
    taken = set()
    _plant_generic(tp, max_doc, taken)
    notes = {"small": [], "both": [], "big": []}
    # tf in {1, 2, 8, 9, 16, 40} in term `big`, the other terms once or twice; a stride of 3 keeps the count at 1 or 2
    d = 3000
    for big in (0, 1):
        for tf in T_SMALL_TFS:
            for twice in (False, True):
                while d in taken:
                    d += 1
                taken.add(d)
                per = _all_terms([20, 23] if twice else [20])
                per[big] = [20 + big + 3 * i for i in range(tf)]
                _plant(tp, d, per)
                notes["small"].append((big, tf, d))
                d += 7
    for tf in T_SMALL_TFS:  # ... and both terms with that tf, every position lined up: count = tf.  Two docs each, of
        for _ in range(2):  # T2's same fieldnorm (doc % 3 != 0): their scores tie, so k = 1 and k = 3 cut through ties
            while d in taken or d % 3 == 0:
                d += 1
            taken.add(d)
            per = _all_terms([20, 23])
            per[0], per[1] = [20 + 3 * i for i in range(tf)], [21 + 3 * i for i in range(tf)]
            _plant(tp, d, per)
            notes["both"].append((tf, d))
            d += 7
    # tf in {254, 255, 256, 300} at every slot of a group of four tf bytes, followed by a plain match in the next posting
    keys = [sorted(t) for t in tp]
    d = 3400
    for big in (0, 1):
        for tf in T_BIG_TFS:
            for slot in range(4):
                while (d in taken or d + 1 in taken or d in tp[big] or d + 1 in tp[big]
                       or bisect.bisect_left(keys[big], d) & 3 != slot):
                    d += 1
                taken.update((d, d + 1))
                per = _all_terms([10, 13])
                per[big] = [10 + big + 3 * i for i in range(tf)]
                _plant(tp, d, per)
                _plant(tp, d + 1, _all_terms([5]))
                for t in range(NT):
                    for x in (d, d + 1):
                        i = bisect.bisect_left(keys[t], x)
                        if i == len(keys[t]) or keys[t][i] != x:
                            keys[t].insert(i, x)
                notes["big"].append((big, tf, slot, d))
                d += 9
    assert d < max_doc
    return tp, max_doc, notes


def build_T():
    tp, max_doc, notes = _build_T_positions()
    return Corpus("T", tp, [40] * max_doc, notes=notes)


def build_T2():
    """T with two fieldnorms: equal scores at the k-th rank and a `min tf` bound that differs between docs."""
    tp, max_doc, notes = _build_T_positions()
    return Corpus("T2", tp, [20 if d % 3 == 0 else 40 for d in range(max_doc)], notes=notes)


# ---- R: repeated positions (leader = term 0, the lowest doc freq)
def build_R():
    rng = np.random.default_rng(1802)
    max_doc = 6000
    tp = _background(rng, max_doc, T_DFS)
    taken = set()
    _plant_generic(tp, max_doc, taken)
    notes = {"rep": []}
    far = [1, 3, 5, 7, 9, 11, 13, 15]  # positions that line up with nothing, in front of the repeats: tf 9
    shapes = [  # (name, term 0, term 1, term 2 relative to p; count of "0 1", count of "0 1 2")
        ("2x1", [0, 0], [1], [2], 1, 1),
        ("2x2", [0, 0], [1, 1], [2], 2, 1),
        ("1x2", [0], [1, 1], [2], 1, 1),
        ("2x3x1", [0, 0], [1, 1, 1], [2], 2, 1),
        ("2x3x2", [0, 0], [1, 1, 1], [2, 2], 2, 2),
    ]
    d = 3000
    for name, a, b, c, c2, c3 in shapes:
        for long_term in (None, 0, 1):  # None: every tf <= 3; else that term has tf 9, repeats included
            for i in range(3):
                while d in taken:
                    d += 1
                taken.add(d)
                p = 40 + 2 * i
                per = _all_terms([p])
                per[0], per[1], per[2] = [p + x for x in a], [p + x for x in b], [p + x for x in c]
                if long_term is not None:  # (the positions in front line up with nothing: the counts stay)
                    per[long_term] = far[: 9 - len(per[long_term])] + per[long_term]
                    assert len(per[long_term]) == 9
                _plant(tp, d, per)
                notes["rep"].append((name, long_term, d, c2, c3))
                d += 11
    return Corpus("R", tp, [40] * max_doc, notes=notes)


# ---- D: where the docs lie
D_DFS = [9000, 18000, 20000, 22000, 24000, 26000, 28000, 30000]
D_MAX_DOC = 70_000
D_EDGE_DOCS = [0, 31, 32, 63, 64, 65535, 65536, D_MAX_DOC - 1]


def _build_D_positions():
    rng = np.random.default_rng(1803)
    tp = _background(rng, D_MAX_DOC, D_DFS)
    taken = set(D_EDGE_DOCS)
    _plant_generic(tp, D_MAX_DOC, taken)
    for i, d in enumerate(D_EDGE_DOCS):
        _plant(tp, d, _all_terms([6, 16] if i % 2 else [6]))
    lead = sorted(tp[0])
    notes = {"lead_127_128": (lead[127], lead[128])}
    for d in notes["lead_127_128"]:  # (docs of the leader already: its posting indices stay)
        assert d not in taken
        _plant(tp, d, _all_terms([9]))
    return tp, notes


def build_D():
    tp, notes = _build_D_positions()
    return Corpus("D", tp, [40] * D_MAX_DOC, notes=notes)


def build_Ddel():
    """D with a third of the docs deleted."""
    tp, notes = _build_D_positions()
    rng = np.random.default_rng(1804)
    deleted = rng.choice(D_MAX_DOC, size=D_MAX_DOC // 3, replace=False)
    return Corpus("Ddel", tp, [40] * D_MAX_DOC, deleted=deleted, notes=notes)


BUILDERS = {"P": build_P, "T": build_T, "T2": build_T2, "R": build_R, "D": build_D, "Ddel": build_Ddel}
CORPORA = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def corpus(name):
    return BUILDERS[name]()
