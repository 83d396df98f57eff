"""Plain numpy models of the tables term preparation derives from a posting list, written from the layouts documented
in tantivy_amd/csrc/tq_device.h (TqdTermHead / TqdTerm / TqdSegment, the range maxima's level rule) and tq_common.hpp
(rdir_lookup), not from the kernels that build them.  Everything is int64 / float64.  A model is a function of
(max_doc, the list's postings, its positions' counts, the fieldnorm ids, the options in force) and, where the device
chose it, of the list's slot / signature bit / shift as tq_term_table_info reports them.

Checked without a GPU by tests/test_prepare_model_cpu.py, compared with the device by tests/test_gpu_prepare_tables.py."""
import numpy as np

TERMINATED = 0x7FFFFFFF
MAT_SLOTS, CLS_SLOTS, SIG_SHIFT, SIG_BITS = 40, 32, 48, 16  # TQD_MAT_SLOTS, TQD_CLS_SLOTS, TQD_SIG_SHIFT, TQD_SIG_BITS
RM_SHIFT, RM_LEVELS = 10, 5                                 # TQD_RM_SHIFT, TQD_RM_LEVELS
RDIR_MIN_DF, RDIR_MIN_DOCS = 256, 4096                      # rdir_plan's floors


def arrays(pl):
    """[(doc, tf)] -> (docs, tfs) as int64"""
    a = np.asarray(pl, np.int64).reshape(-1, 2)
    return a[:, 0].copy(), a[:, 1].copy()


# ---------------------------------------------------------------- the unrolled skip list
def _vint_stop_last(b, at):
    r, shift = 0, 0
    while True:
        v = int(b[at])
        at += 1
        r |= (v & 127) << shift
        if v & 128:
            return r, at
        shift += 7


def skip_entries(list_bytes, df, record_option):
    """The oracle's serialised skip entries of a list (skip.rs:205-253) -> per full block (last_doc, meta, tf_sum), meta
    as rec[j].y packs it: doc_bits | strict << 6 | tf_bits << 8 | block-max fieldnorm id << 16 | block-max tf code << 24."""
    n_full = df // 128
    if not n_full:
        return []
    skip_len, at = _vint_stop_last(list_bytes, 0)
    if skip_len < 8 * n_full:  # (lists written without freqs: block_segment_postings.rs:107-116)
        record_option = 0
    entry = (5, 8, 12)[record_option]
    out = []
    for i in range(n_full):
        e = [int(x) for x in list_bytes[at + entry * i: at + entry * (i + 1)]]
        last = e[0] | e[1] << 8 | e[2] << 16 | e[3] << 24
        doc_bits, strict = e[4] & 0x1F, (e[4] >> 6) & 1
        tf_bits = bm_fn = bm_tf = tf_sum = 0
        if record_option == 1:
            tf_bits, bm_fn, bm_tf = e[5], e[6], e[7]
        elif record_option == 2:
            tf_bits, tf_sum, bm_fn, bm_tf = e[5], e[6] | e[7] << 8 | e[8] << 16 | e[9] << 24, e[10], e[11]
        out.append((last, doc_bits | strict << 6 | tf_bits << 8 | bm_fn << 16 | bm_tf << 24, tf_sum))
    return out


def rec(pl, list_bytes, record_option, with_positions):
    """rec[0 .. n_blocks]: .x the block's last doc, .y the meta word, .z the running 16 * (doc_bits + tf_bits), .w the
    positions before the block; the tail record (.y all ones, .z 0) and the terminator (TERMINATED, 0, 0, every
    position) behind the full blocks."""
    docs, tfs = arrays(pl)
    df = len(docs)
    n_full, n_tail = df // 128, df % 128
    rows, off = [], 0
    for i, (last, meta, _) in enumerate(skip_entries(list_bytes, df, record_option)):
        assert last == docs[128 * i + 127]
        rows.append([last, meta, off, int(tfs[:128 * i].sum()) if with_positions else 0])
        off += 16 * ((meta & 0x1F) + ((meta >> 8) & 0xFF))
    if n_tail:
        rows.append([int(docs[-1]), 0xFFFFFFFF, 0, int(tfs[:128 * n_full].sum()) if with_positions else 0])
    rows.append([TERMINATED, 0, 0, int(tfs.sum()) if with_positions else 0])
    return np.asarray(rows, np.int64)


def tails(pl, has_freq=True):
    docs, tfs = arrays(pl)
    n_full = len(docs) // 128
    t = tfs[128 * n_full:]
    return docs[128 * n_full:], t if has_freq else np.ones_like(t)


def coarse_shift(max_doc, n_blocks):
    """tests/test_term_walk_cpu.py's rule: the smallest shift from 7 that leaves at most two buckets per block (+ 2)"""
    shift = 7
    while ((max_doc - 1) >> shift) + 1 > 2 * n_blocks + 2:
        shift += 1
    return shift


def coarse(max_doc, pl):
    """coarse[b] = the first block whose last doc >= b << shift, one entry past the last bucket as the sentinel"""
    docs, _ = arrays(pl)
    n_blocks = (len(docs) + 127) // 128
    shift = coarse_shift(max_doc, n_blocks)
    block_last = np.append(docs[127::128], docs[-1:] if len(docs) % 128 else [])
    n_buckets = ((max_doc - 1) >> shift) + 1
    return shift, np.searchsorted(block_last, np.arange(n_buckets + 1, dtype=np.int64) << shift, side="left")


# ---------------------------------------------------------------- bitmap, rank directory, bits, directories, bytes
def bitmap_words(max_doc):
    return (max_doc + 31) // 32 + 1


def dense(max_doc, pl):
    """dense[w] = (bits of docs 32 w .. 32 w + 31, postings before word w) over bitmap_words words -> (words, 2)"""
    docs, _ = arrays(pl)
    n = bitmap_words(max_doc)
    bits = np.zeros(n, np.int64)
    np.bitwise_or.at(bits, docs >> 5, np.int64(1) << (docs & 31))
    rank = np.searchsorted(docs, np.arange(n, dtype=np.int64) << 5, side="left")
    return np.stack([bits, rank], axis=1)


def bits(max_doc, pl):
    """the .x halves, zero-padded to a multiple of 256 words"""
    x = dense(max_doc, pl)[:, 0]
    return np.concatenate([x, np.zeros(-len(x) % 256, np.int64)])


def pos_dir(pl):
    """pos_dir[j] = the tfs of postings 0 .. 4 j - 1 together; the last entry holds the total"""
    _, tfs = arrays(pl)
    before = np.concatenate([[0], np.cumsum(tfs)])
    n_dir = (len(tfs) + 3) // 4 + 1
    return before[np.minimum(4 * np.arange(n_dir), len(tfs))]


def tf8(pl):
    return np.minimum(arrays(pl)[1], 255)


def rdir_shift(max_doc, df, dense_ratio=128, dense=True):
    """rdir_plan's rule: no directory for a tiny segment or list (0), else the smallest S in 2..16 that leaves at most df
    ranges of 2^S docs.  (Budgets are not modelled: the tests stay far inside them.)"""
    if not dense or max_doc < RDIR_MIN_DOCS or df < RDIR_MIN_DF:
        return 0
    S = 2
    while S < 16 and (max_doc >> S) + 1 > df:
        S += 1
    return S


def rdir(max_doc, pl, S):
    """-> (dir, entries): dir[r] = postings with doc < r << S for r = 0 .. (max_doc >> S) + 1 (the device pads the
    directory to a multiple of four words; the padding is nobody's), entries (doc & (2^S - 1)) << 16 | min(tf, 0xFFFF)"""
    docs, tfs = arrays(pl)
    r = np.arange((max_doc >> S) + 2, dtype=np.int64)
    return np.searchsorted(docs, r << S, side="left"), (docs & ((1 << S) - 1)) << 16 | np.minimum(tfs, 0xFFFF)


def rdir_dir_words(max_doc, S):
    return ((max_doc >> S) + 2 + 3) & ~3


def rdir_lookup(max_doc, directory, entries, S, d):
    """"is d in the list, with which tf" from the model's tables alone -> min(tf, 0xFFFF) or 0"""
    r = d >> S
    for i in range(int(directory[r]), int(directory[r + 1])):
        if int(entries[i]) >> 16 == d & ((1 << S) - 1):
            return int(entries[i]) & 0xFFFF
    return 0


# ---------------------------------------------------------------- range maxima
def rm_level_entries(max_doc, level):
    return (((max_doc >> (RM_SHIFT + 2 * level)) + 2) + 3) & ~3


def rm_level_off(max_doc, level):
    return sum(rm_level_entries(max_doc, l) for l in range(level))


def rmax_t(pl, fieldnorm_ids, const_id, cache):
    """t = tf / (tf + norm) per posting in float64; norm = the READ-BACK f32 cache entry of the doc's fieldnorm id"""
    docs, tfs = arrays(pl)
    ids = fieldnorm_ids[docs].astype(np.int64) if fieldnorm_ids is not None else np.full(len(docs), const_id, np.int64)
    f = tfs.astype(np.float64)
    return f / (f + np.asarray(cache, np.float64)[ids])


def rmax_byte(t):
    return np.minimum(255, np.floor(255.0 * t).astype(np.int64) + 1)


def rmax(max_doc, pl, fieldnorm_ids, const_id, cache):
    """-> (levels, rmax_list): level 0 a byte per 1024 docs = min(255, floor(255 t) + 1) of the range's largest t, 0
    for a range without a posting; level l + 1 the maximum over four entries of level l; every padding entry 0."""
    docs, _ = arrays(pl)
    q = rmax_byte(rmax_t(pl, fieldnorm_ids, const_id, cache))
    lv = np.zeros(rm_level_entries(max_doc, 0), np.int64)
    np.maximum.at(lv, docs >> RM_SHIFT, q)
    levels = [lv]
    for l in range(1, RM_LEVELS):
        prev = levels[-1]
        nxt = np.zeros(rm_level_entries(max_doc, l), np.int64)
        pooled = np.concatenate([prev, np.zeros(-len(prev) % 4, np.int64)]).reshape(-1, 4).max(axis=1)
        n = min(len(nxt), len(pooled))
        nxt[:n] = pooled[:n]
        levels.append(nxt)
    return levels, int(lv.max()) if len(docs) else 255


def rmax_near_integer(t, eps=1e-4):
    """postings whose 255 t lies within eps of an integer: where an f32 divide may round to the other side"""
    x = 255.0 * t
    return np.abs(x - np.rint(x)) < eps


# ---------------------------------------------------------------- the segment's matrices
def docmat(max_doc, fieldnorm_ids, const_id, columns, signatures):
    """docmat[d]: bits 0..7 the fieldnorm id (or the constant id); bit 8 + slot iff d is in the list that owns the slot
    (columns: {slot: postings}); bit 48 + b iff d is in at least one of the lists given signature bit b (signatures:
    [(b, postings)]); every other bit zero.  uint64."""
    m = (fieldnorm_ids.astype(np.uint64) if fieldnorm_ids is not None else np.full(max_doc, const_id, np.uint64)).copy()
    for slot, pl in columns.items():
        assert 0 <= slot < MAT_SLOTS
        m[arrays(pl)[0]] |= np.uint64(1) << np.uint64(8 + slot)
    for b, pl in signatures:
        assert 0 <= b < SIG_BITS
        m[arrays(pl)[0]] |= np.uint64(1) << np.uint64(SIG_SHIFT + b)
    return m


def doccls(max_doc, columns):
    """doccls[d] = 2 bits per slot below TQD_CLS_SLOTS: 0 absent, 1 or 2 = the tf, 3 = three or more.  uint64."""
    m = np.zeros(max_doc, np.uint64)
    for slot, pl in columns.items():
        if slot < CLS_SLOTS:
            docs, tfs = arrays(pl)
            m[docs] |= np.minimum(tfs, 3).astype(np.uint64) << np.uint64(2 * slot)
    return m


def lnorm(pl, fieldnorm_ids):
    """the fieldnorm ids in posting order, 128 bytes per block, zero bytes behind the last posting of the last block"""
    docs, _ = arrays(pl)
    out = np.zeros((len(docs) + 127) // 128 * 128, np.int64)
    out[:len(docs)] = fieldnorm_ids[docs]
    return out


def flat(pl):
    """tq_xunion.hip's plain arrays -> (doc ids, offset of the tf bytes = the doc ids padded to 16 bytes, min(tf, 255))"""
    docs, tfs = arrays(pl)
    return docs, (4 * len(docs) + 15) & ~15, np.minimum(tfs, 255)
