"""The plain-Python codec model (tests/codec_model.py) equals the oracle byte for byte on the
directed inputs of tests/encode_cases.py, and every input reaches the code it was made for.  The
GPU tests (test_gpu_encode_edges.py) run the same inputs through tq_encode.hip."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import codec_model as M
from tests import encode_cases as K


def _same_postings(case):
    want, want_ts = O.serialize_postings_batch(*case)
    got, got_ts = M.serialize_postings_batch(*case)
    assert np.array_equal(got_ts, want_ts), K.first_diff(got_ts, want_ts)
    assert K.first_diff(got, want) is None, K.first_diff(got, want)
    return want, want_ts


def _same_positions(case):
    want, want_ts = O.serialize_positions_batch(*case)
    got, got_ts = M.serialize_positions_batch(*case)
    assert np.array_equal(got_ts, want_ts), K.first_diff(got_ts, want_ts)
    assert K.first_diff(got, want) is None, K.first_diff(got, want)


def test_fieldnorm_table_matches_the_oracle():
    import ctypes as C

    L = O.lib()
    L.to_id_to_fieldnorm.restype = C.c_uint32
    assert [M.fieldnorm_of(i) for i in range(256)] == [L.to_id_to_fieldnorm(C.c_uint8(i)) for i in range(256)]


@pytest.mark.parametrize("record_option", K.RECORD_OPTIONS)
@pytest.mark.parametrize("descending", [False, True])
def test_width_matrix(descending, record_option):
    case = K.width_matrix(descending, record_option)
    _same_postings(case)
    hit = K.postings_widths(case)
    assert {d for d, _ in hit} == set(range(32))
    if record_option != K.BASIC:
        assert {t for _, t in hit} == set(K.TF_WIDTHS)
    doc_al, tf_al = K.postings_alignments(case)
    assert doc_al == {0, 1, 2, 3}
    if record_option != K.BASIC:
        assert tf_al == {0, 1, 2, 3}
    assert K.wide_then_narrow(case) >= (16 if descending else 1)
    assert int(case[1].max()) <= K.MAX_DOC


@pytest.mark.parametrize("descending", [False, True])
def test_position_widths(descending):
    case = K.position_widths(descending)
    _same_positions(case)
    assert K.positions_widths_hit(case) == set(range(33))
    assert K.positions_alignments(case) == {0, 1, 2, 3}
    tails = {int(n) % 128 for n in np.diff(case[0].astype(np.int64)) if n >= 256}
    assert tails == set(K.TAIL_LENGTHS)


@pytest.mark.parametrize("record_option", K.RECORD_OPTIONS)
def test_vint_edges(record_option):
    case = K.vint_edges(record_option)
    _same_postings(case)
    lens = K.vint_lengths(case)
    assert lens["delta"] == {1, 2, 3, 4, 5}
    if record_option != K.BASIC:
        assert lens["tf"] == {1, 2, 3, 4, 5}
    sizes = np.diff(case[0].astype(np.int64))
    assert {int(n) for n in sizes if n < 128} == set(K.TAIL_LENGTHS)
    assert {int(n) % 128 for n in sizes if n >= 128} == set(K.TAIL_LENGTHS)  # tails after full blocks
    assert int(case[1].max()) == K.MAX_DOC


def test_vint_edges_positions():
    case = K.vint_edges_positions()
    _same_positions(case)
    assert K.vint_lengths(case)["delta"] == {1, 2, 3, 4, 5}
    assert int(case[1].max()) == K.U32_MAX


@pytest.mark.parametrize("record_option", K.RECORD_OPTIONS)
def test_header_edges_around_128(record_option):
    case = K.header_edges(record_option, 128)
    _same_postings(case)
    lo, hi = K.skip_lens(case)
    assert lo < 128 <= hi


@pytest.mark.parametrize("record_option", K.RECORD_OPTIONS)
def test_header_edges_around_16384_straddle(record_option):
    """(Too many blocks for the model; the GPU test compares these with the oracle.)"""
    lo, hi = K.skip_lens(K.header_edges(record_option, 16384))
    assert lo < 16384 <= hi


def test_header_edges_positions():
    case = K.header_edges_positions(128)
    _same_positions(case)
    assert [int(n) // 128 for n in np.diff(case[0].astype(np.int64))] == [127, 128]
    big = K.header_edges_positions(16384)
    assert [int(n) // 128 for n in np.diff(big[0].astype(np.int64))] == [16383, 16384]


@pytest.mark.parametrize("record_option", K.RECORD_OPTIONS)
def test_first_blocks(record_option):
    case = K.first_blocks(record_option)
    _same_postings(case)
    ts, docs = case[0].astype(np.int64), case[1]
    assert (np.diff(ts)[:70] == 128).all() and (np.diff(ts)[70:] == 256).all()
    assert set(docs[ts[:-1]].tolist()) == {0, 1}
    assert (docs[ts[1:-1] - 1] > 1_000_000).all()  # the value before every first doc is high


def _skip_pairs(body, body_ts, case):
    """The block-max (fieldnorm id, tf code) bytes of every skip entry, in output order."""
    entry = K.HEADER_ROWS[case[6]][0]
    out = []
    for t in range(len(case[0]) - 1):
        n_full = int(case[0][t + 1] - case[0][t]) // 128
        if not n_full:
            continue
        at = int(body_ts[t]) + len(M.vint_stop_last(n_full * entry))
        for j in range(n_full):
            e = body[at + j * entry: at + (j + 1) * entry]
            out.append((int(e[-2]), int(e[-1])))
    return out


@pytest.mark.parametrize("record_option", [K.WITH_FREQS, K.WITH_FREQS_AND_POSITIONS])
@pytest.mark.parametrize("avg", K.AVGS)
def test_block_max_ties(avg, record_option):
    case = K.block_max_ties(avg, record_option)
    body, body_ts = _same_postings(case)
    prof = K.tie_profile(case)
    wrote = _skip_pairs(body, body_ts, case)
    assert len(wrote) == len(prof)
    for (t, first, last, n_distinct), got in zip(prof, wrote):
        assert got == (last[0], min(last[1], 255)), (t, first, last, got)
        if t < 3:  # the tie blocks: a first-wins writer would store another fieldnorm id
            assert n_distinct >= 2 and first[0] != last[0], (t, first, last)
    # the one-maximum blocks of term 3 (index 0, index 127) have exactly one maximal pair
    assert [n for t, _, _, n in prof if t == 3] == [1, 1]
    tf, fn = case[2], case[3]
    assert int(tf[: int(case[0][1])].min()) >= 1 << 26 and int(fn[:1024].max()) < 40
    near = case[2][int(case[0][K.TIE_TERMS]):]
    assert near.min() >= 1 << 20 and near.max() < (1 << 20) + 128
    if avg == 37.25:  # the oracle's answer on this input, found on the CPU before any kernel ran
        assert [p[0] for p in wrote[:2]] == [21, 5]
        assert [f for _, f, _, _ in prof[:2]] == [(0, 1 << 26), (24, (1 << 26) + 128)]


@pytest.mark.parametrize("record_option", K.RECORD_OPTIONS)
@pytest.mark.parametrize("target", [4095, 4096, 4097])
def test_scan_shapes_small(target, record_option):
    case = K.scan_shapes(target, record_option)
    _same_postings(case)
    assert K.n_items_partials(case[0]) == (target, 1 if target == 4095 else 2)


@pytest.mark.parametrize("target", [4095, 4096, 4097])
def test_scan_shapes_small_positions(target):
    case = K.scan_shapes_positions(target)
    _same_positions(case)
    assert K.n_items_partials(case[0])[0] == target


def test_scan_shapes_reach_the_scan_paths():
    """n_items exactly 4095 / 4096 / 4097 (4096: the total's slot is alone in the second tile), a
    few tiles, and more than 256 partials with more terms than the capped grid has wavefronts."""
    assert [K.n_items_partials(K.scan_shapes_positions(t)[0]) for t in K.SCAN_TARGETS] == [
        (4095, 1), (4096, 2), (4097, 2), (20_000, 5)]
    ts = K.scan_shapes_positions(K.SCAN_LARGE)[0]
    n_items, n_partials = K.n_items_partials(ts)
    assert n_items > 1_048_576 and n_partials == 257
    assert len(ts) - 1 > 8192 * 4  # the term loops stride
    sizes = np.diff(ts.astype(np.int64))
    assert set(sizes.tolist()) == {0, 1, 2, 3, 128, 129, 130}


def test_tie_inputs_tell_the_last_maximum_from_the_first(monkeypatch):
    """A writer that keeps the FIRST maximum differs from the oracle on the tie input, in the
    fieldnorm byte of every tie block's skip entry: the input decides the rule."""
    case = K.block_max_ties(37.25, K.WITH_FREQS)
    want, want_ts = O.serialize_postings_batch(*case)

    def first_wins(fids, tfs, cache):
        best, pair = None, (0, 0)
        for fid, tf in zip(fids, tfs):
            s = np.float32(tf) / (np.float32(tf) + cache[fid])
            if best is None or s > best:
                best, pair = s, (int(fid), int(tf))
        return pair

    monkeypatch.setattr(M, "block_max_pair", first_wins)
    got, got_ts = M.serialize_postings_batch(*case)
    assert np.array_equal(got_ts, want_ts) and got.size == want.size
    a, b = _skip_pairs(got, got_ts, case), _skip_pairs(want, want_ts, case)
    assert [x[0] for x in a[:4]] == [0, 24, 64 % 40, 1] and [x[0] for x in b[:4]] == [21, 5, 65 % 40, 128 % 40]
    # the one-maximum blocks do not depend on the rule
    assert a[4:6] == b[4:6]
