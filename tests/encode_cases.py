"""Directed inputs for the codec writers (tq_encode.hip), shared by the CPU test of the model and
the GPU tests of the encoder, with the pure functions that say what each input is for.

A postings case is (term_starts, docs, tfs, fieldnorm_ids, num_docs, avg, record_option); a
positions case is (term_starts, deltas).  Seeds are fixed; doc ids stay at or below MAX_DOC."""
import numpy as np

BASIC, WITH_FREQS, WITH_FREQS_AND_POSITIONS = 0, 1, 2
RECORD_OPTIONS = (BASIC, WITH_FREQS, WITH_FREQS_AND_POSITIONS)
MAX_DOC = 0x7FFFFFFE
U32_MAX = 0xFFFFFFFF
SCAN_TILE = 4096  # items per tile of the scan kernels

TF_WIDTHS = (0, 1, 7, 8, 9, 31, 32)
TAIL_LENGTHS = (1, 63, 64, 65, 127)
VINT_EDGES = (127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21, (1 << 28) - 1, 1 << 28)
AVGS = (0.0078125, 37.25, 1e6)


def _assemble(doc_lists, tf_lists=None):
    ts = np.cumsum([0] + [len(l) for l in doc_lists]).astype(np.uint64)
    cat = lambda ls: (np.concatenate([np.asarray(l, np.uint64) for l in ls]).astype(np.uint32)
                      if ls else np.zeros(0, np.uint32))
    docs = cat(doc_lists)
    if tf_lists is None:
        return ts, docs
    return ts, docs, cat(tf_lists)


def _docs_from_strict(strict):
    """strict[0] is the first doc, strict[i] = doc[i] - doc[i-1] - 1."""
    d = np.cumsum(np.asarray(strict, np.int64) + 1) - 1
    assert d[-1] <= MAX_DOC
    return d


def _tfs_of_width(rng, n, width, spots):
    """n tfs whose tf - 1 needs exactly `width` bits, the widest value at every index of spots."""
    if width == 0:
        return np.ones(n, np.int64)
    top = U32_MAX if width == 32 else (1 << width)  # 0xFFFFFFFF - 1 has 32 bits
    t = rng.integers(0, min(1 << width, 1 << 12), size=n).astype(np.int64) + 1
    t[list(spots)] = top
    return t


# ---------------------------------------------------------------------------- width_matrix
def width_matrix(descending, record_option):
    """One term of two full blocks per doc width 0..31, tf widths cycling through TF_WIDTHS, filler
    terms of 1, 2 and 3 docs in between so that payloads start at every byte alignment.  Both blocks
    hold the width's largest delta 2^w - 1, as far as doc ids allow: two deltas of width 30 or 31 do
    not fit below 2^31 in one list.  The term of width 30 has 2^30 - 1 in its first block and
    2^30 - 2^20 in its second; width 31 gets two terms, one with its 31-bit delta in the first block
    (the raw first doc) and one with it in the second, the other block having width 0."""
    rng = np.random.default_rng(4100)
    terms = []  # (docs, tfs)
    specs = [(w, 0) for w in range(32)] + [(31, 1)]
    for k, (w, where31) in enumerate(specs):
        p1, p2 = (5 * w + 3) % 128, 128 + (11 * w + 64) % 128
        if w == 0:
            strict = np.zeros(256, np.int64)
        elif w <= 29:
            strict = rng.integers(0, min(1 << w, 1 << 16), size=256).astype(np.int64)
            strict[[p1, p2]] = (1 << w) - 1
        elif w == 30:
            strict = rng.integers(0, 1 << 10, size=256).astype(np.int64)
            strict[p1], strict[p2] = (1 << 30) - 1, (1 << 30) - (1 << 20)
        else:
            strict = np.zeros(256, np.int64)
            strict[p2 if where31 else p1] = MAX_DOC - 255
        tw = TF_WIDTHS[k % len(TF_WIDTHS)]
        terms.append((_docs_from_strict(strict), _tfs_of_width(rng, 256, tw, (p1, p2))))
    if descending:
        terms.reverse()
    doc_lists, tf_lists = [], []
    for k, (d, t) in enumerate(terms):
        doc_lists.append(d)
        tf_lists.append(t)
        n = 1 + k % 3
        first = (0, 200, 20_000)[(k // 3) % 3]  # vints of 1, 2 and 3 bytes
        doc_lists.append(first + 2 * np.arange(n))
        tf_lists.append(np.array([1, 130, 3][:n]))
    ts, docs, tfs = _assemble(doc_lists, tf_lists)
    return ts, docs, tfs, None, 0, 0.0, record_option


def postings_widths(case):
    """The (doc width, tf width) of every full block, from the inputs alone (tf width 0 without freqs)."""
    ts, docs, tfs, _, _, _, opt = case
    hit = set()
    for t in range(len(ts) - 1):
        lo, hi = int(ts[t]), int(ts[t + 1])
        for j in range((hi - lo) // 128):
            b = docs[lo + 128 * j: lo + 128 * (j + 1)].astype(np.int64)
            prev = np.concatenate([[docs[lo + 128 * j - 1] if j else -1], b[:-1]])
            doc_bits = int(np.bitwise_or.reduce((b - prev - 1) & U32_MAX)).bit_length()
            tf_bits = 0
            if opt != BASIC:
                f = tfs[lo + 128 * j: lo + 128 * (j + 1)].astype(np.int64)
                tf_bits = int(np.bitwise_or.reduce((f - 1) & U32_MAX)).bit_length()
            hit.add((doc_bits, tf_bits))
    return hit


def postings_alignments(case):
    """(off & 3 of the doc payloads, off & 3 of the tf payloads), over blocks whose payload is not
    empty, from the model's layout."""
    from tests import codec_model as M

    lay = M.postings_layout(*case)
    return ({d & 3 for _, _, d, db, _, _ in lay if db}, {f & 3 for _, _, _, _, f, fb in lay if fb})


def wide_then_narrow(case):
    """Number of blocks whose payload is shorter than that of the block before it (in output order,
    which is the order a wavefront walks them): where stale words of the staging buffer would show."""
    from tests import codec_model as M

    ws = [db + fb for _, _, _, db, _, fb in M.postings_layout(*case)]
    return sum(1 for a, b in zip(ws, ws[1:]) if b < a)


# ---------------------------------------------------------------------------- position_widths
def position_widths(descending):
    """One term per width 0..32 of the positions file: two full blocks that both hold the width's
    largest value, then a tail of 1, 63, 64, 65 or 127 values; fillers of 1, 2 and 3 values between."""
    rng = np.random.default_rng(4200)
    terms = []
    for w in range(33):
        n = 256 + TAIL_LENGTHS[w % 5]
        v = rng.integers(0, min(1 << w, 1 << 16), size=n).astype(np.int64) if w else np.zeros(n, np.int64)
        if w:
            v[[(5 * w + 3) % 128, 128 + (11 * w + 64) % 128]] = (1 << w) - 1
        v[256:] = rng.integers(0, 1 << 15, size=n - 256)  # the tail is free of the block widths
        terms.append(v)
    if descending:
        terms.reverse()
    lists = []
    for k, v in enumerate(terms):
        lists.append(v)
        lists.append(np.array([5, 300, 70_000][: 1 + k % 3]))
    return _assemble(lists)


def positions_widths_hit(case):
    ts, deltas = case
    hit = set()
    for t in range(len(ts) - 1):
        lo, hi = int(ts[t]), int(ts[t + 1])
        for j in range((hi - lo) // 128):
            hit.add(int(np.bitwise_or.reduce(deltas[lo + 128 * j: lo + 128 * (j + 1)])).bit_length())
    return hit


def positions_alignments(case):
    from tests import codec_model as M

    return {off & 3 for _, _, off, b in M.positions_layout(*case) if b}


# ---------------------------------------------------------------------------- vint_edges
def _edge_deltas(n, s, largest):
    """n plain deltas: the small edges in rotation, 2^28 - 1 and 2^28 once each where they fit, and
    (for s odd) the largest value that still fits as the last one."""
    d = [VINT_EDGES[(i + s) % 6] for i in range(n)]
    if n >= 63:
        a = (17 * s) % n
        d[a] = (1 << 28) - 1
        d[(a + n // 2 + 1) % n] = 1 << 28  # one of the two lies past index 63 when n > 64
    if s % 2:
        d[-1] = largest - (sum(d) - d[-1])
    return d


def vint_edges(record_option):
    """Tails of 1, 63, 64, 65 and 127 postings (twice each: 64 is where a lane's second value starts)
    whose doc deltas and tfs sit on the vint length boundaries, then the same tails after one and two
    full blocks, so that the first delta of the tail counts from the last doc of the block before."""
    doc_lists, tf_lists = [], []
    s = 0
    for n_full in (0, 0, 1, 2):
        for n in TAIL_LENGTHS:
            head = 1000 * s + 3 * np.arange(128 * n_full)  # full blocks first
            last = int(head[-1]) if n_full else 0
            d = _edge_deltas(n, s, MAX_DOC - last)
            doc_lists.append(np.concatenate([head, last + np.cumsum(d)]).astype(np.int64))
            assert doc_lists[-1][-1] <= MAX_DOC
            tf = [(VINT_EDGES + (U32_MAX,))[(i + 2 * s) % 9] for i in range(128 * n_full + n)]
            tf_lists.append(np.array(tf, np.int64))
            s += 1
    ts, docs, tfs = _assemble(doc_lists, tf_lists)
    return ts, docs, tfs, None, 0, 0.0, record_option


def vint_edges_positions():
    lists = []
    s = 0
    for n_full in (0, 1, 2):
        for n in TAIL_LENGTHS:
            v = [(VINT_EDGES + (U32_MAX,))[(i + s) % 9] for i in range(128 * n_full + n)]
            lists.append(np.array(v, np.int64))
            s += 1
    return _assemble(lists)


def _vint_len(v):
    v = np.asarray(v, np.int64)
    return 1 + (v >= 1 << 7).astype(int) + (v >= 1 << 14) + (v >= 1 << 21) + (v >= 1 << 28)


def vint_lengths(case):
    """The vint lengths of the tails: {"delta": set, "tf": set} for postings, {"delta": set} for positions."""
    positions = len(case) == 2
    ts, vals = case[0], case[1]
    out = {"delta": set()} if positions else {"delta": set(), "tf": set()}
    for t in range(len(ts) - 1):
        lo, hi = int(ts[t]), int(ts[t + 1])
        cut = lo + (hi - lo) // 128 * 128
        if cut == hi:
            continue
        v = vals[cut:hi].astype(np.int64)
        if not positions:
            v = np.diff(v, prepend=int(vals[cut - 1]) if cut > lo else 0)
            if case[6] != BASIC:
                out["tf"] |= set(_vint_len(case[2][cut:hi]).tolist())
        out["delta"] |= set(_vint_len(v).tolist())
    return out


# ---------------------------------------------------------------------------- header_edges
HEADER_ROWS = {  # record option -> (skip entry size, n_full around 128, n_full around 16 384)
    BASIC: (5, (25, 26), (3276, 3277)),
    WITH_FREQS: (8, (15, 16), (2047, 2048)),
    WITH_FREQS_AND_POSITIONS: (12, (10, 11), (1365, 1366)),
}


def header_edges(record_option, around):
    """Two terms whose skip_len = n_full * entry size lies just below and just at or above `around`
    (128 or 16 384), so that VInt(skip_len) grows by a byte between them.  Most blocks are
    consecutive docs with tf 1 (width 0); every 7th has gaps and every 5th has tfs up to 4."""
    rng = np.random.default_rng(4300 + record_option)
    _, small, large = HEADER_ROWS[record_option]
    doc_lists, tf_lists = [], []
    for n_full in (small if around == 128 else large):
        n = 128 * n_full + 5
        gaps = np.ones(n, np.int64)
        tf = np.ones(n, np.int64)
        for j in range(0, n_full, 7):
            gaps[128 * j + int(rng.integers(0, 128))] += int(rng.integers(1, 1 << (1 + j % 9)))
        for j in range(0, n_full, 5):
            tf[128 * j: 128 * j + 128] = rng.integers(1, 5, size=128)
        gaps[0] = int(rng.integers(0, 2))  # first doc 0 or 1
        doc_lists.append(np.cumsum(gaps))
        tf_lists.append(tf)
    ts, docs, tfs = _assemble(doc_lists, tf_lists)
    num_docs = int(docs.max()) + 1
    fn = rng.integers(0, 256, size=num_docs).astype(np.uint8)
    return ts, docs, tfs, fn, num_docs, 37.25, record_option


def header_edges_positions(around):
    """Position terms with 127 / 128 or 16383 / 16384 full blocks: VInt(n_full) grows by a byte."""
    rng = np.random.default_rng(4400)
    lists = []
    for n_full in ((127, 128) if around == 128 else (16383, 16384)):
        v = np.zeros(128 * n_full + 3, np.int64)
        for j in range(0, n_full, 9):
            v[128 * j: 128 * j + 128] = rng.integers(0, 1 << (1 + j % 11), size=128)
        v[-3:] = (1, 200, 70_000)
        lists.append(v)
    return _assemble(lists)


def skip_lens(case):
    entry = HEADER_ROWS[case[6]][0]
    return [int(case[0][t + 1] - case[0][t]) // 128 * entry for t in range(len(case[0]) - 1)]


# ---------------------------------------------------------------------------- first_blocks
def first_blocks(record_option):
    """70 terms of exactly 128 docs (every block is the first of its term), then three of 256.  Every
    term starts at doc 0 or 1 right after a term that ended near the top of the doc range: the value
    before a term's first one must not leak into its first delta."""
    rng = np.random.default_rng(4500)
    num_docs = 1 << 20
    doc_lists, tf_lists = [], []
    for t in range(73):
        n = 128 if t < 70 else 256
        rest = np.sort(rng.choice(np.arange(2, num_docs - 100), size=n - 2, replace=False))
        doc_lists.append(np.concatenate([[t % 2], rest, [num_docs - 1 - t]]))
        tf_lists.append(rng.integers(1, 20, size=n))
    ts, docs, tfs = _assemble(doc_lists, tf_lists)
    fn = rng.integers(0, 256, size=num_docs).astype(np.uint8)
    return ts, docs, tfs, fn, num_docs, 37.25, record_option


# ---------------------------------------------------------------------------- block_max_ties
def _scores(case):
    from tests import codec_model as M

    ts, docs, tfs, fn, _, avg, _ = case
    cache = np.array(M.tf_cache(avg), np.float32)
    t = tfs.astype(np.float32)
    with np.errstate(all="ignore"):
        return t / (t + cache[fn[docs]])


def exact_tie_ids(avg, tf_lo, tf_hi):
    """How many leading fieldnorm ids 0..m-1 (m <= 40) give a score of exactly 1.0f for every tf of
    [tf_lo, tf_hi): tf + cache[id] rounds back to tf."""
    from tests import codec_model as M

    cache = M.tf_cache(avg)
    m = 0
    with np.errstate(all="ignore"):
        while m < 40 and all(np.float32(tf) + cache[m] == np.float32(tf) for tf in (tf_lo, tf_hi - 1)):
            m += 1
    return m


TIE_TERMS = 4  # the first terms of block_max_ties are the tie blocks; the rest are near-ties


def block_max_ties(avg, record_option):
    """Blocks whose block-max pair depends on the tie rule.  Term 0: the issue's input, 256 docs
    0, 3, 6, ... with distinct tfs >= 2^26 and fieldnorm id = doc % m: every score is exactly 1.0f,
    every pair is distinct.  (m = 40 where every id below 40 ties at tf 2^26; for the smallest avg
    the cache is so large that only the first few ids tie, at tfs just below 2^32.)  Term 1: a block whose
    maximum is at index 63 and, with another pair, at index 64.  Term 2: the same two pairs at
    indices 0 and 127.  Term 3: one block with its only maximum at index 0, one with it at index
    127.  Terms 4..: dense near-ties, tf in [2^20, 2^20 + 128) and fieldnorm ids below 24."""
    rng = np.random.default_rng(4600)
    tf_base = 1 << 26
    m = exact_tie_ids(avg, tf_base, tf_base + 256)
    if m < 2:
        tf_base = (1 << 32) - 512
        m = exact_tie_ids(avg, tf_base, tf_base + 256)
    assert m >= 2, (avg, m)
    num_docs = 4096
    fn = np.empty(num_docs, np.uint8)
    fn[:1024] = np.arange(1024) % m
    fn[1024:] = rng.integers(0, 24, size=num_docs - 1024)
    doc_lists = [3 * np.arange(256)]
    tf_lists = [tf_base + np.arange(256)]
    for a, b in ((63, 64), (0, 127)):
        doc_lists.append(1 + np.arange(128))
        tf = rng.integers(1, 6, size=128)
        tf[a], tf[b] = tf_base + 1, tf_base + 2
        tf_lists.append(tf)
    doc_lists.append(2 + 2 * np.arange(256))
    tf = rng.integers(1, 6, size=256)
    tf[0], tf[255] = tf_base + 7, tf_base + 9
    tf_lists.append(tf)
    for _ in range(2):
        doc_lists.append(np.sort(rng.choice(np.arange(1024, num_docs), size=256, replace=False)))
        tf_lists.append((1 << 20) + rng.integers(0, 128, size=256))
    ts, docs, tfs = _assemble(doc_lists, tf_lists)
    return ts, docs, tfs, fn, num_docs, avg, record_option


def tie_profile(case):
    """Per full block, in output order: (term, first maximal pair, last maximal pair, number of
    distinct maximal pairs), pairs being (fieldnorm id, tf) and the scores f32."""
    ts, docs, tfs, fn, _, _, _ = case
    s = _scores(case)
    out = []
    for t in range(len(ts) - 1):
        lo, hi = int(ts[t]), int(ts[t + 1])
        for j in range((hi - lo) // 128):
            sl = slice(lo + 128 * j, lo + 128 * (j + 1))
            at = np.nonzero(s[sl] == s[sl].max())[0] + sl.start
            pairs = [(int(fn[docs[i]]), int(tfs[i])) for i in at]
            out.append((t, pairs[0], pairs[-1], len(set(pairs))))
    return out


# ---------------------------------------------------------------------------- scan_shapes
SCAN_TARGETS = (4095, 4096, 4097, 20_000)
SCAN_LARGE = 1_049_000


def _scan_sizes(n_items_target):
    """Term sizes with n_blocks + 2 * n_terms == n_items_target exactly: tiny terms of 0..3 values
    and a one-block term of 128..130 values about every 1000 terms."""
    n_big = max(1, n_items_target // 2048)
    if (n_items_target - n_big) % 2:
        n_big += 1
    n_terms = (n_items_target - n_big) // 2
    sizes = np.arange(n_terms, dtype=np.int64) % 4
    at = (np.arange(n_big) * (n_terms // n_big)) + min(7, n_terms // n_big - 1)
    sizes[at] = 128 + np.arange(n_big) % 3
    return sizes


def scan_shapes(n_items_target, record_option):
    rng = np.random.default_rng(4700)
    sizes = _scan_sizes(n_items_target)
    ts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(ts[-1])
    term = np.repeat(np.arange(sizes.size), sizes)
    within = np.arange(n) - ts[:-1].astype(np.int64)[term]
    base = (term * 37) % 60_000  # first doc deltas of 1, 2 and 3 vint bytes
    docs = (base + 3 * within + (within > 1) * 200).astype(np.uint32)
    tfs = rng.integers(1, 300, size=n).astype(np.uint32)
    num_docs = 1 << 16
    fn = rng.integers(0, 256, size=num_docs).astype(np.uint8)
    assert int(docs.max()) < num_docs
    return ts, docs, tfs, fn, num_docs, 37.25, record_option


def scan_shapes_positions(n_items_target):
    rng = np.random.default_rng(4800)
    sizes = _scan_sizes(n_items_target)
    ts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    deltas = rng.integers(0, 1 << 9, size=int(ts[-1])).astype(np.uint32)
    deltas[::11] = rng.integers(1 << 14, 1 << 22, size=deltas[::11].size)
    return ts, deltas


def n_items_partials(term_starts):
    """(n_items, n_partials) as the encoder counts them: one item per full block, two per term;
    tiles of 4096 over n_items + 1 slots (the last holds the total)."""
    sizes = np.diff(np.asarray(term_starts, np.uint64).astype(np.int64))
    n_items = int((sizes // 128).sum()) + 2 * sizes.size
    return n_items, (n_items + 1 + SCAN_TILE - 1) // SCAN_TILE


def first_diff(got, want):
    """None when equal, else a short report of the first differing offsets."""
    got, want = np.asarray(got), np.asarray(want)
    if got.size != want.size:
        n = min(got.size, want.size)
        bad = np.nonzero(got[:n] != want[:n])[0]
        return "length %d != %d, first differing offsets %s" % (got.size, want.size, bad[:10].tolist())
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return None
    return "%d differ, first offsets %s: got %s want %s" % (
        bad.size, bad[:10].tolist(), got[bad[:10]].tolist(), want[bad[:10]].tolist())
