"""A plain-Python writer of the postings (.idx body) and positions (.pos) bytes, for small inputs.

It restates, independently of the oracle's C code, what the reference's PostingsSerializer
(src/postings/serializer.rs), SkipSerializer (src/postings/skip.rs), PositionSerializer
(src/positions/serializer.rs) and the vint block codec (src/postings/compression/vint.rs) write
for a batch of terms.  Bit-packing and vints come from tests/helpers (pack4x, vint_stop_last).

One posting list:
  * Docs and term frequencies are buffered 128 at a time.  A full buffer becomes one block: the
    doc ids as "strict" deltas (doc - previous - 1, wrapping in 32 bits; the very first doc of a
    term is stored as it is, because the serializer starts every term with "no previous doc",
    which it spells as a last encoded doc of 0), bit-packed at the width of the OR of the deltas;
    then, if the field records frequencies, tf - 1 bit-packed at its own width.
  * Every block appends one skip entry: last doc (u32 LE), doc width with bit 6 set (the
    strict-delta flag), and with frequencies: tf width, [sum of the block's tfs as u32 LE when
    positions are recorded], then the block-max pair: fieldnorm id and tf (saturated at 255) of the
    posting with the largest tf / (tf + cache[fieldnorm id]), computed in f32; among equal scores
    the LAST posting wins (Iterator::max_by).  Without fieldnorms (or with num_docs == 0) the pair is (0, 0).
  * What is left at the end of the term (fewer than 128 postings) is written as vints: plain
    deltas doc - previous (previous = last doc of the last block, or 0), then the tfs.
  * The term's bytes are [VInt(len(skip)) skip] (only when it has at least 128 docs), blocks, tail.

One position list: blocks of 128 deltas bit-packed at the width of their OR, the remainder as
vints; the term's bytes are VInt(number of full blocks), one width byte per block, the payload.

Both functions have the call shape of oracle.serialize_postings_batch / serialize_positions_batch
and return (np.uint8 bytes, np.uint64 term starts).  Speed is no concern: directed inputs only.
"""
import numpy as np

from tests.helpers import pack4x, vint_stop_last

BASIC, WITH_FREQS, WITH_FREQS_AND_POSITIONS = 0, 1, 2
BLOCK = 128
M32 = 0xFFFFFFFF


def fieldnorm_of(fid):
    """Fieldnorm ids below 24 are the fieldnorm itself; above, every step of 8 ids doubles the
    spacing (a 3-bit mantissa with an implied leading one), starting at 24."""
    if fid < 24:
        return fid
    b = fid - 24
    mant, exp = b & 7, b >> 3
    return 24 + (mant if exp == 0 else (mant | 8) << (exp - 1))


def tf_cache(avg):
    """cache[id] = K1 * (1 - B + B * fieldnorm(id) / avg), every step rounded to f32."""
    f = np.float32
    out = []
    with np.errstate(all="ignore"):
        for fid in range(256):
            x = f(0.75) * f(fieldnorm_of(fid))
            x = x / f(avg)
            x = (f(1.0) - f(0.75)) + x
            out.append(f(1.2) * x)
    return out


def block_max_pair(fids, tfs, cache):
    """(fieldnorm id, tf) of the best posting of a block; a later posting replaces the current best
    unless its score is strictly less."""
    f = np.float32
    best = None
    pair = (0, 0)
    with np.errstate(all="ignore"):
        for fid, tf in zip(fids, tfs):
            t = f(tf)
            s = t / (t + cache[fid])
            if best is None or not (s < best):
                best, pair = s, (int(fid), int(tf))
    return pair


def _bits(vals):
    acc = 0
    for v in vals:
        acc |= v
    return acc.bit_length()


def _u32le(v):
    return int(v).to_bytes(4, "little")


def _postings(term_starts, docs, tfs, fieldnorm_ids, num_docs, avg, record_option, layout):
    has_freq = record_option != BASIC
    has_pos = record_option == WITH_FREQS_AND_POSITIONS
    has_bm25 = has_freq and fieldnorm_ids is not None and num_docs > 0
    cache = tf_cache(avg) if has_bm25 else None
    out = bytearray()
    starts = []
    ts = [int(x) for x in term_starts]
    for t in range(len(ts) - 1):
        starts.append(len(out))
        d = [int(x) for x in docs[ts[t]: ts[t + 1]]]
        f = [int(x) for x in tfs[ts[t]: ts[t + 1]]] if has_freq else None
        skip, body, metas = bytearray(), bytearray(), []
        last = 0
        n_full = len(d) // BLOCK
        for j in range(n_full):
            bd = d[BLOCK * j: BLOCK * (j + 1)]
            prev = last if last != 0 else None
            deltas = []
            for v in bd:
                deltas.append(v if prev is None else (v - prev - 1) & M32)
                prev = v
            last = bd[-1]
            doc_bits = _bits(deltas)
            skip += _u32le(last) + bytes([doc_bits | 0x40])
            doc_at = len(body)
            body += pack4x(deltas, doc_bits)
            tf_bits, tf_at = 0, len(body)
            if has_freq:
                bt = f[BLOCK * j: BLOCK * (j + 1)]
                m1 = [(x - 1) & M32 for x in bt]
                tf_bits = _bits(m1)
                body += pack4x(m1, tf_bits)
                skip.append(tf_bits)
                if has_pos:
                    skip += _u32le(sum(bt) & M32)
                fid, btf = (0, 0)
                if has_bm25:
                    fid, btf = block_max_pair([int(fieldnorm_ids[v]) for v in bd], bt, cache)
                skip += bytes([fid, min(btf, 255)])
            metas.append((j, doc_at, doc_bits, tf_at, tf_bits))
        tail = bytearray()
        for v in d[BLOCK * n_full:]:
            tail += vint_stop_last((v - last) & M32)
            last = v
        if has_freq:
            for x in f[BLOCK * n_full:]:
                tail += vint_stop_last(x)
        head = (vint_stop_last(len(skip)) + bytes(skip)) if len(d) >= BLOCK else b""
        if layout is not None:
            at = len(out) + len(head)
            for j, doc_at, doc_bits, tf_at, tf_bits in metas:
                layout.append((t, j, at + doc_at, doc_bits, at + tf_at, tf_bits))
        out += head + body + tail
    starts.append(len(out))
    return np.frombuffer(bytes(out), np.uint8).copy(), np.array(starts, np.uint64)


def serialize_postings_batch(term_starts, docs, tfs, fieldnorm_ids, num_docs, avg_fieldnorm,
                             record_option):
    return _postings(term_starts, docs, tfs, fieldnorm_ids, num_docs, avg_fieldnorm, record_option,
                     None)


def postings_layout(term_starts, docs, tfs, fieldnorm_ids, num_docs, avg_fieldnorm, record_option):
    """Where the model puts every full block: (term, block in term, offset of the doc payload, doc
    width, offset of the tf payload, tf width)."""
    layout = []
    _postings(term_starts, docs, tfs, fieldnorm_ids, num_docs, avg_fieldnorm, record_option, layout)
    return layout


def _positions(term_starts, deltas, layout):
    out = bytearray()
    starts = []
    ts = [int(x) for x in term_starts]
    for t in range(len(ts) - 1):
        starts.append(len(out))
        d = [int(x) for x in deltas[ts[t]: ts[t + 1]]]
        n_full = len(d) // BLOCK
        widths, body, metas = bytearray(), bytearray(), []
        for j in range(n_full):
            blk = d[BLOCK * j: BLOCK * (j + 1)]
            b = _bits(blk)
            widths.append(b)
            metas.append((j, len(body), b))
            body += pack4x(blk, b)
        for v in d[BLOCK * n_full:]:
            body += vint_stop_last(v)
        head = vint_stop_last(n_full) + bytes(widths)
        if layout is not None:
            for j, at, b in metas:
                layout.append((t, j, len(out) + len(head) + at, b))
        out += head + body
    starts.append(len(out))
    return np.frombuffer(bytes(out), np.uint8).copy(), np.array(starts, np.uint64)


def serialize_positions_batch(term_starts, deltas):
    return _positions(term_starts, deltas, None)


def positions_layout(term_starts, deltas):
    """(term, block in term, offset of the payload, width) of every full block."""
    layout = []
    _positions(term_starts, deltas, layout)
    return layout
