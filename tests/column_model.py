"""A plain-Python writer and reader of the reference's u64_based column-values bytes, and the range decision over them.

It restates, independently of the library's C++ and HIP code, what serialize_u64_based_column_values writes and
load_u64_based_column_values reads (columnar/src/column_values/u64_based/{mod,bitpacked,linear,blockwise_linear,line}.rs,
columnar/src/column_values/stats.rs, bitpacker/src/{bitpacker,lib}.rs):

  blob      one codec byte (0 Bitpacked, 1 Linear, 2 BlockwiseLinear), ColumnStats, the codec's payload.
  stats     four VInts (7 bits per byte, low bits first, bit 7 set on the LAST byte): min, gcd, (max - min) / gcd, rows.
  bit pack  value i occupies `width` bits at bit i * width of a little-endian stream, low bit first; the stream ends on a
            byte border.  A reader takes the 8 bytes at byte (i * width) >> 3 (missing ones read as 0), shifts them right by
            (i * width) & 7 and masks `width` bits — which is why widths 57..63 do not exist: compute_num_bits gives
            the bit length of its argument, or 64 when that exceeds 56.
  line      slope and intercept as two VInts; eval(x) = intercept + sign_extend_32((x * slope mod 2^64) >> 32), all mod
            2^64: a falling line's slope is 2^64 - 1 - |slope|.
  Bitpacked payload = (value - min) / gcd packed at compute_num_bits((max - min) / gcd) bits.
  Linear    payload = Line, a width byte, value - eval(row) (mod 2^64) packed at that width; min and gcd play no part.
  Blockwise payload = per block of 512 rows, n = (value - min) / gcd as n - eval(row % 512) packed at the block's own
            width, the blocks end to end (block b starts at byte sum of width * 64 of the blocks before it); then a footer of
            (Line, width byte) per block; then the footer's length as u32 LE.  value = min + gcd * (eval + diff).

Only the READERS' arithmetic is normative; the writers pick a line through a block's first and last value, as the
reference's Line::train does, and an intercept that makes every stored difference non-negative.

expected_range() is search_on_u64_ff + bound_to_value_range (src/query/range_query/range_query_fastfield.rs:414-503) over
plain Python ints, with the library's documented answer for the reference's EmptyScorer (an empty set scoring the boost).
Speed: numpy where a column has 10^5 rows; the scalar functions next to them are the literal restatement the CPU tests
hold the vectorised ones against."""
import functools
import math

import numpy as np

BITPACKED, LINEAR, BLOCKWISE = 0, 1, 2
FULL, OPTIONAL, MULTIVALUED = 0, 1, 2
BLOCK = 512
M64 = (1 << 64) - 1
U64 = np.uint64


# ---- VInt, stats, compute_num_bits
def vint(v):
    out = bytearray()
    while True:
        b = v & 127
        v >>= 7
        if v == 0:
            out.append(b | 128)
            return bytes(out)
        out.append(b)


def read_vint(data, at):
    v, shift = 0, 0
    while True:
        b = data[at]
        at += 1
        v |= (b & 127) << shift
        if b & 128:
            return v, at
        shift += 7


def compute_num_bits(n):
    bits = int(n).bit_length()
    return bits if bits <= 56 else 64


def stats_of(values):
    """(min, max, gcd, rows) of a column as the reference's stats collector leaves them (no rows: 0, 0, 1, 0; all equal: gcd 1)."""
    vals = [int(v) for v in values]
    if not vals:
        return 0, 0, 1, 0
    lo, hi = min(vals), max(vals)
    g = functools.reduce(math.gcd, (v - lo for v in vals), 0)
    return lo, hi, g or 1, len(vals)


def stats_bytes(lo, hi, gcd, rows):
    return vint(lo) + vint(gcd) + vint((hi - lo) // gcd) + vint(rows)


# ---- the bit packer
def pack(ns, width):
    """BitPacker::write for every n, then close."""
    if width == 0 or len(ns) == 0:
        return b""
    a = np.array([int(n) for n in ns], dtype=U64) if not isinstance(ns, np.ndarray) else ns.astype(U64)
    bits = ((a[:, None] >> np.arange(width, dtype=U64)[None, :]) & U64(1)).astype(np.uint8)
    return np.packbits(bits.reshape(-1), bitorder="little").tobytes()


def unpack_one(data, idx, width):
    """BitUnpacker::get, literally."""
    if width == 0:
        return 0
    addr_in_bits = idx * width
    addr = addr_in_bits >> 3
    eight = bytes(data[addr: addr + 8]).ljust(8, b"\0")
    mask = M64 if width == 64 else (1 << width) - 1
    return (int.from_bytes(eight, "little") >> (addr_in_bits & 7)) & mask


def unpack(data, n, width):
    """Rows 0..n-1 at once -> uint64 array."""
    if width == 0 or n == 0:
        return np.zeros(n, U64)
    bits = np.unpackbits(np.frombuffer(bytes(data), np.uint8), bitorder="little")
    need = n * width
    if bits.size < need:
        bits = np.concatenate([bits, np.zeros(need - bits.size, np.uint8)])
    m = bits[:need].reshape(n, width).astype(U64)
    return (m << np.arange(width, dtype=U64)[None, :]).sum(axis=1, dtype=U64)


# ---- Line
def line_eval(slope, intercept, x):
    lin = ((x * slope) & M64) >> 32 & 0xFFFFFFFF
    if lin & 0x80000000:
        lin -= 1 << 32
    return (intercept + lin) & M64


def line_eval_np(slope, intercept, xs):
    with np.errstate(over="ignore"):
        lin = ((xs.astype(U64) * U64(slope)) >> U64(32)).astype(np.uint32).astype(np.int32).astype(np.int64).astype(U64)
        return U64(intercept) + lin


def train_line(ys):
    """A valid Line for the values `ys` (Python ints mod 2^64) and the non-negative differences it leaves:
    compute_slope through the first and last value, then the intercept that makes the smallest difference 0."""
    n = len(ys)
    slope = 0
    if n > 1:
        dy = (ys[-1] - ys[0]) & M64
        rising = dy <= 1 << 63
        abs_dy = dy if rising else (ys[0] - ys[-1]) & M64
        if abs_dy < 1 << 31:
            abs_slope = (abs_dy << 32) // (n - 1)
            slope = abs_slope if rising else M64 - abs_slope
    raw = [(y - line_eval(slope, 0, i)) & M64 for i, y in enumerate(ys)]
    rel = [((r - raw[0] + (1 << 63)) & M64) - (1 << 63) for r in raw]  # signed distance from the first difference
    low = min(rel)
    intercept = (raw[0] + low) & M64
    return slope, intercept, [r - low for r in rel]


# ---- writers
def write_bitpacked(values):
    lo, hi, g, rows = stats_of(values)
    width = compute_num_bits((hi - lo) // g)
    return bytes([BITPACKED]) + stats_bytes(lo, hi, g, rows) + pack([(int(v) - lo) // g for v in values], width)


def write_linear(values):
    lo, hi, g, rows = stats_of(values)
    slope, intercept, diffs = train_line([int(v) for v in values]) if rows else (0, 0, [])
    width = compute_num_bits(max(diffs)) if diffs else 0
    return bytes([LINEAR]) + stats_bytes(lo, hi, g, rows) + vint(slope) + vint(intercept) + bytes([width]) + pack(diffs, width)


def write_blockwise(values):
    lo, hi, g, rows = stats_of(values)
    ns = [(int(v) - lo) // g for v in values]
    data, footer = bytearray(), bytearray()
    for b in range(0, rows, BLOCK):
        slope, intercept, diffs = train_line(ns[b: b + BLOCK])
        width = compute_num_bits(max(diffs))
        data += pack(diffs, width)  # (a full block is width * 64 bytes: the next one starts on a byte border)
        footer += vint(slope) + vint(intercept) + bytes([width])
    return bytes([BLOCKWISE]) + stats_bytes(lo, hi, g, rows) + bytes(data) + bytes(footer) + len(footer).to_bytes(4, "little")


WRITERS = {BITPACKED: write_bitpacked, LINEAR: write_linear, BLOCKWISE: write_blockwise}


# ---- reader
def read_header(blob):
    """-> dict(codec, min_value, max_value, gcd, num_rows, num_bits, at): the fields of the header; num_bits 0 for the
    linear codecs; at = where the codec's payload starts."""
    codec = blob[0]
    lo, at = read_vint(blob, 1)
    g, at = read_vint(blob, at)
    amp, at = read_vint(blob, at)
    rows, at = read_vint(blob, at)
    return {"codec": codec, "min_value": lo, "max_value": lo + amp * g, "gcd": g, "num_rows": rows,
            "num_bits": compute_num_bits(amp) if codec == BITPACKED else 0, "at": at}


def block_widths(blob):
    """The bit widths of a BlockwiseLinear blob's blocks."""
    return [w for _, _, w in _blocks(blob, read_header(blob))]


def _blocks(blob, h):
    footer_len = int.from_bytes(blob[-4:], "little")
    at = len(blob) - 4 - footer_len
    out = []
    for _ in range((h["num_rows"] + BLOCK - 1) // BLOCK):
        slope, at = read_vint(blob, at)
        intercept, at = read_vint(blob, at)
        out.append((slope, intercept, blob[at]))
        at += 1
    return out


def read_column(blob):
    """Every row's value -> uint64 array (vectorised)."""
    h = read_header(blob)
    rows, at, lo, g = h["num_rows"], h["at"], h["min_value"], h["gcd"]
    with np.errstate(over="ignore"):
        if h["codec"] == BITPACKED:
            return U64(lo) + U64(g) * unpack(blob[at:], rows, h["num_bits"])
        if h["codec"] == LINEAR:
            slope, at = read_vint(blob, at)
            intercept, at = read_vint(blob, at)
            width = blob[at]
            return line_eval_np(slope, intercept, np.arange(rows)) + unpack(blob[at + 1:], rows, width)
        out = np.zeros(rows, U64)
        off = at
        for b, (slope, intercept, width) in enumerate(_blocks(blob, h)):
            n = min(BLOCK, rows - b * BLOCK)
            ns = line_eval_np(slope, intercept, np.arange(n)) + unpack(blob[off: off + (n * width + 7) // 8], n, width)
            out[b * BLOCK: b * BLOCK + n] = U64(lo) + U64(g) * ns
            off += width * BLOCK // 8
        return out


def read_one(blob, row):
    """One row's value, scalar arithmetic only (the literal get_val of the three readers)."""
    h = read_header(blob)
    at, lo, g = h["at"], h["min_value"], h["gcd"]
    if h["codec"] == BITPACKED:
        return lo + g * unpack_one(blob[at:], row, h["num_bits"])
    if h["codec"] == LINEAR:
        slope, at = read_vint(blob, at)
        intercept, at = read_vint(blob, at)
        return (line_eval(slope, intercept, row) + unpack_one(blob[at + 1:], row, blob[at])) & M64
    blocks = _blocks(blob, h)
    footer_at = len(blob) - 4 - int.from_bytes(blob[-4:], "little")
    off = at + sum(w * BLOCK // 8 for _, _, w in blocks[: row // BLOCK])
    slope, intercept, width = blocks[row // BLOCK]
    n = (line_eval(slope, intercept, row % BLOCK) + unpack_one(blob[off:footer_at], row % BLOCK, width)) & M64
    return (lo + g * n) & M64


# ---- the range decision
def value_range(lower, upper, lo, hi):
    """bound_to_value_range: (start, end) or None for an overflowing Excluded bound.  A bound: None, ("in", v), ("ex", v)."""
    if lower is None:
        start = lo
    elif lower[0] == "in":
        start = lower[1]
    else:
        if lower[1] == M64:
            return None
        start = lower[1] + 1
    start = max(start, lo)
    if upper is None:
        end = hi
    elif upper[0] == "in":
        end = upper[1]
    else:
        if upper[1] == 0:
            return None
        end = upper[1] - 1
    return start, end


def expected_range(values, present, lower, upper, boost):
    """-> ("all" | "set", mask over the docs, weight).  values: one per ROW; present: None (a Full column: row = doc) or a
    bool array over the docs (an Optional column: the rows are the present docs in order)."""
    vals = np.array([int(v) for v in values], dtype=object) if not isinstance(values, np.ndarray) else values
    max_doc = len(vals) if present is None else len(present)
    if lower is None and upper is None:
        return "all", np.ones(max_doc, bool), 1.0
    lo, hi, _, rows = stats_of(vals) if vals.dtype == object else _np_stats(vals)
    empty = ("set", np.zeros(max_doc, bool), float(boost))
    r = value_range(lower, upper, lo, hi)
    if r is None or rows == 0:
        return empty
    start, end = r
    if start > end or start > hi or end < lo:
        return empty
    if present is None and lo >= start and hi <= end and float(boost) == 1.0:
        return "all", np.ones(max_doc, bool), 1.0
    if vals.dtype == object:
        hit = np.array([start <= int(v) <= end for v in vals], bool)
    else:
        hit = (vals >= U64(start)) & (vals <= U64(min(end, M64)))
    mask = np.zeros(max_doc, bool)
    if present is None:
        mask[:] = hit
    else:
        mask[np.nonzero(present)[0]] = hit
    return "set", mask, float(boost)


def _np_stats(vals):
    if vals.size == 0:
        return 0, 0, 1, 0
    return int(vals.min()), int(vals.max()), 1, int(vals.size)


def bound_table(lo, hi, gcd, mid_a, mid_b):
    """The bounds every column is asked: (name, lower, upper, boost).  lo / hi / gcd: the column's stats; mid_a <= mid_b: two
    values between them."""
    t = [
        ("both unbounded, boost 2", None, None, 2.0),
        ("lower Excluded(u64::MAX)", ("ex", M64), None, 1.0),
        ("upper Excluded(0)", None, ("ex", 0), 1.0),
        ("upper Excluded(min)", None, ("ex", lo), 1.5),
        ("lower Excluded(max)", ("ex", hi), None, 1.0),
        ("lo == hi at min", ("in", lo), ("in", lo), 1.0),
        ("lo == hi at max", ("in", hi), ("in", hi), 0.5),
        ("lo == hi in the middle", ("in", mid_a), ("in", mid_a), 1.0),
        ("start > end", ("in", mid_b), ("ex", mid_b), 1.0),
        ("a middle range", ("in", mid_a), ("in", mid_b), 1.0),
        ("a middle range, exclusive, boost 2.5", ("ex", mid_a), ("ex", mid_b), 2.5),
        ("ends off the gcd grid", ("in", min(mid_a + 1, M64)), ("in", max(mid_b - 1, 0)), 1.0),
        ("ends off the gcd grid, outwards", ("ex", max(mid_a - 1, 0)), ("ex", min(mid_b + 1, M64)), 1.0),
        ("all but min", ("ex", lo), None, 1.0),
        ("all but max", None, ("ex", hi), 1.0),
        ("covering, boost 1", ("in", lo), ("in", hi), 1.0),
        ("covering, boost 2", ("in", lo), ("in", hi), 2.0),
        ("covering from 0 to u64::MAX, boost 1", ("in", 0), ("in", M64), 1.0),
        ("covering, lower unbounded, boost 2", None, ("in", M64), 2.0),
    ]
    if lo > 0:
        t.append(("end < min", ("in", 0), ("in", lo - 1), 1.0))
    if hi < M64:
        t.append(("start > max", ("in", hi + 1), ("in", M64), 1.0))
    return t


def expected_table(mask):
    """The {32 doc bits, docs before the word} table of a doc mask, its sentinel entry {0, docs} included -> (words + 1, 2) uint32."""
    n_words = (mask.size + 31) // 32
    padded = np.zeros(n_words * 32, np.uint8)
    padded[: mask.size] = mask
    words = np.packbits(padded, bitorder="little").view(np.uint32) if n_words else np.zeros(0, np.uint32)
    pops = padded.reshape(n_words, 32).sum(axis=1, dtype=np.uint64) if n_words else np.zeros(0, np.uint64)
    ranks = np.concatenate([[0], np.cumsum(pops)]).astype(np.uint32)
    return np.stack([np.concatenate([words, [0]]).astype(np.uint32), ranks], axis=1)


def presence_words(present):
    """A bool array over the docs as the uint32 words tq_column_upload takes."""
    n_words = (present.size + 31) // 32
    padded = np.zeros(n_words * 32, np.uint8)
    padded[: present.size] = present
    return np.packbits(padded, bitorder="little").view(np.uint32).copy() if n_words else np.zeros(0, np.uint32)
