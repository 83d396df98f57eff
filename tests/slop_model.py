"""A plain model of PhraseQuery with slop > 0 (PhraseScorer with has_slop(), src/query/phrase_query/phrase_scorer.rs;
the list order of Intersection::new, src/query/intersection.rs), written from the behaviour: what each step keeps, in
which order, and where it stops.  Token-level input as tests/phrase_model.py: per term {doc: [positions]}.

What a sloppy phrase is NOT: an exact phrase with a window.  Five properties decide every verdict:

  1. the lists are walked in COST order — doc freq ascending, ties in phrase order (a stable sort) — not phrase order;
  2. positions are adjusted: position + max(offsets) - offset of the term, distances are |a - b| on adjusted positions;
  3. two terms: one streaming two-pointer walk (pair_count / pair_exists).  Three and more: the middle lists are folded
     into a CARRIED list of (position, slop spent) by carry_step, the last list is then counted by carry_step without
     a new list (scoring) or tested by pair_exists, which forgets the slop already spent (not scoring);
  4. so the scored and the unscored verdict of one doc may differ for three and more terms;
  5. the carried list is deduplicated against its last entry only: it may hold repeats, be non-monotone, and has no bound.
     The slop spent is kept in a byte.

Part 2 turns the per-doc verdicts into doc sets, BM25 scores (phrase_model's helpers) and top-k rows."""
import numpy as np

from tests import phrase_model as PM


# ------------------------------------------------------------------------------------------------ 1. per doc
def pair_count(left, right, slop):
    """Two lists, scoring: matches counted by one walk.  After a match the left cursor first moves to the last left
    value that is not beyond the right value, then both move on by one."""
    li = ri = n = 0
    while li < len(left) and ri < len(right):
        a, b = left[li], right[ri]
        if abs(a - b) <= slop:
            while li + 1 < len(left) and left[li + 1] <= b:
                li += 1
            n += 1
            li += 1
            ri += 1
        elif a < b:
            li += 1
        else:
            ri += 1
    return n


def pair_merge(left, right, slop):
    """The same walk keeping the matched RIGHT values: what the reference's update_left leaves in `left`."""
    li = ri = 0
    kept = []
    while li < len(left) and ri < len(right):
        a, b = left[li], right[ri]
        if abs(a - b) <= slop:
            while li + 1 < len(left) and left[li + 1] <= b:
                li += 1
            kept.append(b)
            li += 1
            ri += 1
        elif a < b:
            li += 1
        else:
            ri += 1
    return kept


def pair_exists(left, right, slop):
    """Two lists, not scoring: is there a pair within the slop on the two-pointer path."""
    li = ri = 0
    while li < len(left) and ri < len(right):
        a, b = left[li], right[ri]
        if abs(a - b) <= slop:
            return True
        if a < b:
            li += 1
        else:
            ri += 1
    return False


class _Carry:
    """The list a carry step builds: a value equal to the LAST one kept only lowers that entry's slop."""

    def __init__(self):
        self.pos, self.spent = [], []

    def add(self, spent, value):
        spent &= 0xFF  # (a byte: slops above 255 wrap in the reference; the device refuses them)
        if self.pos and self.pos[-1] == value:
            self.spent[-1] = min(self.spent[-1], spent)
        else:
            self.pos.append(value)
            self.spent.append(spent)


def carry_step(left, spent, right, slop):
    """One list folded into the carried one.  -> (matches, new positions, new slops).  `spent` may be shorter than
    `left` (the first list: nothing spent yet)."""
    if not left or not right:
        return 0, [], []
    at = lambda i: spent[i] if i < len(spent) else 0
    out = _Carry()
    li = ri = n = 0
    while True:
        a, sa, b = left[li], at(li), right[ri]
        d = sa + abs(a - b)
        if d <= slop:
            # both values stay, and every value of the smaller one's list up to the larger one: which is the best
            # partner is only known at the next list
            small_is_left = a < b
            walk, i = (left, li) if small_is_left else (right, ri)
            large = b if small_is_left else a
            cur = d
            out.add(cur, a if small_is_left else b)
            while i + 1 < len(walk) and walk[i + 1] <= large:
                i += 1
                cur = sa + abs(walk[i] - large)
                out.add(cur, walk[i])
            out.add(cur, large)
            n += 1
            li += 1
            ri += 1
        elif a < b:
            li += 1
        else:
            ri += 1
        if li >= len(left):  # the rest of the right list against the LAST left value
            a, sa = left[-1], (spent[-1] if spent else 0)
            for b in right[ri:]:
                d = abs(a - b) + sa
                if d <= slop:
                    out.add(d, b)
            break
        if ri >= len(right):  # the rest of the left list against the LAST right value
            b = right[-1]
            for i in range(li, len(left)):
                d = abs(left[i] - b) + at(i)
                if d <= slop:
                    out.add(d, left[i])
            break
    return n, out.pos, out.spent


class DocVerdict:
    __slots__ = ("count", "exists", "longest")

    def __init__(self, count, exists, longest):
        self.count, self.exists, self.longest = count, exists, longest


def doc_verdict(lists, slop):
    """lists: the adjusted positions of one doc per term IN COST ORDER.  -> the scored count, the unscored verdict and
    the longest initial or carried list met (0 for two terms: nothing is carried)."""
    assert slop >= 1 and len(lists) >= 2
    if len(lists) == 2:
        return DocVerdict(pair_count(lists[0], lists[1], slop), pair_exists(lists[0], lists[1], slop), 0)
    left, spent = list(lists[0]), []
    longest = len(left)
    for right in lists[1:-1]:
        _, left, spent = carry_step(left, spent, right, slop)
        longest = max(longest, len(left))
        if not left:
            return DocVerdict(0, False, longest)
    count = carry_step(left, spent, lists[-1], slop)[0]
    return DocVerdict(count, pair_exists(left, lists[-1], slop), longest)


def fold_reference_style(lists, slop):
    """The reference's unit-test harness of the carry step: every list after the first folded with update_left, the
    slops starting as zeros.  -> (count of the last step, [(slop, position)])."""
    left, spent, n = list(lists[0]), [0] * len(lists[0]), 0
    for right in lists[1:]:
        n, left, spent = carry_step(left, spent, list(right), slop)
    return n, list(zip(spent, left))


# ------------------------------------------------------------------------------------------------ 2. per query
def cost_order(term_positions, terms):
    """Indices into `terms` in the order the lists are walked: doc freq ascending, ties in phrase order."""
    return sorted(range(len(terms)), key=lambda i: len(PM._lists(term_positions, terms[i])))


def adjusted_lists(term_positions, terms, offsets, doc, order=None):
    top = max(offsets)
    order = cost_order(term_positions, terms) if order is None else order
    return [[p + top - offsets[i] for p in term_positions[terms[i]][doc]] for i in order]


def verdicts(term_positions, terms, offsets, slop, alive=None, order=None):
    """{doc: DocVerdict} over the candidates (the alive docs that hold every term)."""
    order = cost_order(term_positions, terms) if order is None else order
    return {d: doc_verdict(adjusted_lists(term_positions, terms, offsets, d, order), slop)
            for d in PM.and_docs(term_positions, terms, alive)}


class SlopExpect:
    """What the model says of one query: the scored rows (docs ascending, float64 scores, counts), the unscored doc set
    and the longest carried list over its candidates."""

    def __init__(self, term_positions, terms, offsets, slop, fieldnorms, alive=None):
        v = verdicts(term_positions, terms, offsets, slop, alive)
        max_doc = len(fieldnorms)
        self.longest = max((x.longest for x in v.values()), default=0)
        self.longest_doc = max(v, key=lambda d: v[d].longest) if v else None
        self.docs = np.array(sorted(d for d, x in v.items() if x.count > 0), np.uint32)
        self.counts = np.array([v[int(d)].count for d in self.docs], np.int64)
        self.exists_docs = np.array(sorted(d for d, x in v.items() if x.exists), np.uint32)
        avgdl = float(sum(int(f) for f in fieldnorms)) / max_doc
        w = PM.phrase_weight(term_positions, terms, max_doc)
        self.scores = np.array([PM.bm25(w, int(c), float(fieldnorms[int(d)]), avgdl) for d, c in zip(self.docs, self.counts)],
                               np.float64)

    def top_k(self, k):
        return PM.top_k(self.docs, self.scores, k)
