"""Model of TopDocs::order_by_fast_field on one segment, written from the reference's sources (read, not copied):

* the segment sort key is Column<u64>::first(doc) = Option<u64> (src/collector/sort_key/sort_by_static_fast_value.rs:62-96);
* the four comparators (src/collector/sort_key/order.rs:68-221) are two independent choices — descending / ascending, and
  docs without a value last / first: Natural = (desc, last), ReverseNoneLower = (asc, last), Reverse = (asc, first),
  NaturalNoneHigher = (desc, first); Order::Asc -> ReverseNoneLower, Order::Desc -> Natural (:286-293);
* compare_for_top_k (src/collector/top_score_collector.rs:503-683): the comparator on the key, reversed, then ascending doc
  id whatever the order.

`expected_sorted` is the closed form: the alive matching docs ordered by (class, value', doc), the first min(k, matches)
of them.  `TopNComputer` is a literal transliteration of the reference's buffer (capacity 2 * max(k, 1), truncation at the
median of the buffer — the element of index k under compare_for_top_k —, a strict threshold, into_sorted_vec), fed in
ascending doc order as default_collect_segment_impl does.  tests/test_sort_model_cpu.py shows that the two agree.

Everything is in Python ints, so that 2^64 - 1 is exact."""
import functools

DESC, ASC = 0, 1           # tq_sort_order
NULLS_LAST, NULLS_FIRST = 0, 1  # tq_sort_nulls
U64 = (1 << 64) - 1
COMPARATORS = {"Natural": (DESC, NULLS_LAST), "ReverseNoneLower": (ASC, NULLS_LAST), "Reverse": (ASC, NULLS_FIRST),
               "NaturalNoneHigher": (DESC, NULLS_FIRST)}


def rank_key(value, order, nulls):
    """(class, value') of an Option<u64> (None: no value); SMALLER comes first in the result."""
    if value is None:
        return (0 if nulls == NULLS_FIRST else 2, 0)
    v = int(value)
    return (1, v if order == ASC else U64 - v)


def per_doc_values(values, present):
    """Column<u64>::first(doc) of every doc as a list of Python ints / None: values[row] for row = the rank of a doc among
    the docs with a value (present: bool per doc, or None: every doc has a value and row = doc)."""
    if present is None:
        return [int(v) for v in values]
    out, r = [], 0
    for p in present:
        out.append(int(values[r]) if p else None)
        r += 1 if p else 0
    return out


def expected_sorted_docs(match_docs, per_doc, k, order, nulls):
    """The closed form over per_doc_values: -> [(doc, value or None)], the first min(k, matches)."""
    keyed = sorted(rank_key(per_doc[int(d)], order, nulls) + (int(d),) for d in match_docs)
    return [(key[2], per_doc[key[2]]) for key in keyed[: int(k)]]


def expected_sorted(match_docs, values, present, k, order, nulls):
    """match_docs: the alive matching docs; values / present as per_doc_values takes them.  -> [(doc, value or None)]"""
    return expected_sorted_docs(match_docs, per_doc_values(values, present), k, order, nulls)


# ---- the reference's comparators on Option<u64>, as Ordering of (lhs, rhs): -1 Less, 0 Equal, 1 Greater
def _cmp(a, b):
    return (a > b) - (a < b)


def _option_cmp(a, b):
    """Option<u64>'s derived Ord: None < Some(_)."""
    if a is None or b is None:
        return _cmp(a is not None, b is not None)
    return _cmp(a, b)


def comparator_compare(name, lhs, rhs):
    if name == "Natural":                 # lhs.partial_cmp(rhs)
        return _option_cmp(lhs, rhs)
    if name == "Reverse":                 # rhs.partial_cmp(lhs)
        return _option_cmp(rhs, lhs)
    if name == "ReverseNoneLower":        # reversed on values, None still the lowest
        if lhs is None or rhs is None:
            return _cmp(lhs is not None, rhs is not None)
        return _cmp(rhs, lhs)
    assert name == "NaturalNoneHigher"    # natural on values, None the highest
    if lhs is None or rhs is None:
        return _cmp(lhs is None, rhs is None)
    return _cmp(lhs, rhs)


def compare_for_top_k(name, lhs, rhs):
    """lhs / rhs = (sort_key, doc).  The comparator on the keys, REVERSED (the best comes first), then ascending doc."""
    c = -comparator_compare(name, lhs[0], rhs[0])
    return c if c else _cmp(lhs[1], rhs[1])


class TopNComputer:
    """The reference's TopNComputer: a buffer of 2 * max(top_n, 1) entries; push drops what does not beat the threshold
    (strictly), a full buffer is truncated to its top_n best by selecting the element of index top_n and keeping what
    comes before it; the threshold becomes that median element."""

    def __init__(self, top_n, comparator):
        self.top_n = top_n
        self.cap = 2 * max(top_n, 1)
        self.name = comparator
        self.buffer = []
        self.has_threshold = False  # (the threshold is an Option<Score> and a Score may itself be None)
        self.threshold = None

    def _cmp_entries(self, a, b):
        return compare_for_top_k(self.name, a, b)

    def push(self, sort_key, doc):
        if self.has_threshold:
            # strict: a key that does not compare Greater than the last median is dropped
            if comparator_compare(self.name, sort_key, self.threshold) != 1:
                return
        if len(self.buffer) == self.cap:
            self.threshold = self._truncate_top_n()
            self.has_threshold = True
        self.buffer.append((sort_key, doc))

    def _truncate_top_n(self):
        # select_nth_unstable_by(top_n, compare_for_top_k): any arrangement with the element of sorted index top_n in
        # place, the better ones before it; a full sort is one such arrangement
        self.buffer.sort(key=functools.cmp_to_key(self._cmp_entries))
        median = self.buffer[self.top_n]
        del self.buffer[self.top_n:]
        return median[0]

    def into_sorted_vec(self):
        if len(self.buffer) > self.top_n:
            self._truncate_top_n()
        self.buffer.sort(key=functools.cmp_to_key(self._cmp_entries))
        return list(self.buffer)


def top_n_reference(match_docs, values, present, k, comparator):
    """collect_segment_top_k: every alive matching doc in ascending doc order through TopNComputer.  -> [(doc, value | None)]"""
    per_doc = per_doc_values(values, present)
    top = TopNComputer(int(k), comparator)
    for d in sorted(int(x) for x in match_docs):
        top.push(per_doc[d], d)
    return [(doc, key) for key, doc in top.into_sorted_vec()]
