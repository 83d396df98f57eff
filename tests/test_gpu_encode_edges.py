"""The device-side codec writers (tq_encode.hip) on the directed inputs of tests/encode_cases.py:
the scan over several tiles, the grid-stride loops, the block-max tie rule, every width, alignment
and vint length, the device entry points into a poisoned buffer, a reused encoder, argument errors.
Bytes and term starts must equal the oracle's and, on the small inputs, the plain-Python model's."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import codec_model as M
from tests import encode_cases as K

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 64


@pytest.fixture(scope="module")
def ta():
    import tantivy_amd

    return tantivy_amd


@pytest.fixture(scope="module")
def enc(ta):
    e = ta.Encoder(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def _postings(builder, *args):
    """(case, oracle bytes, oracle term starts), computed once and shared; nobody writes to them."""
    case = getattr(K, builder)(*args)
    return (case,) + O.serialize_postings_batch(*case)


@functools.lru_cache(maxsize=None)
def _positions(builder, *args):
    case = getattr(K, builder)(*args)
    return (case,) + O.serialize_positions_batch(*case)


def _expect(got, got_ts, want, want_ts, what=""):
    assert np.array_equal(got_ts, want_ts), (what, K.first_diff(got_ts, want_ts))
    diff = K.first_diff(got, want)
    assert diff is None, (what, diff)


def _encode(enc, case):
    if len(case) == 2:
        return enc.encode_positions(*case)
    ts, docs, tfs = case[:3]
    return enc.encode_postings(ts, docs, None if case[6] == K.BASIC else tfs, *case[3:])


def _check_postings(enc, builder, *args, model=True):
    case, want, want_ts = _postings(builder, *args)
    got, got_ts = _encode(enc, case)
    _expect(got, got_ts, want, want_ts, "oracle")
    if model:
        _expect(got, got_ts, *M.serialize_postings_batch(*case), "model")


def _check_positions(enc, builder, *args, model=True):
    case, want, want_ts = _positions(builder, *args)
    got, got_ts = _encode(enc, case)
    _expect(got, got_ts, want, want_ts, "oracle")
    if model:
        _expect(got, got_ts, *M.serialize_positions_batch(*case), "model")


# ------------------------------------------------------------------ the cases, host entry points
@pytest.mark.parametrize("record_option", K.RECORD_OPTIONS)
@pytest.mark.parametrize("descending", [False, True])
def test_width_matrix(enc, descending, record_option):
    _check_postings(enc, "width_matrix", descending, record_option)


@pytest.mark.parametrize("descending", [False, True])
def test_position_widths(enc, descending):
    _check_positions(enc, "position_widths", descending)


@pytest.mark.parametrize("record_option", K.RECORD_OPTIONS)
def test_vint_edges(enc, record_option):
    _check_postings(enc, "vint_edges", record_option)


def test_vint_edges_positions(enc):
    _check_positions(enc, "vint_edges_positions")


@pytest.mark.parametrize("around", [128, 16384])
@pytest.mark.parametrize("record_option", K.RECORD_OPTIONS)
def test_header_edges(enc, record_option, around):
    _check_postings(enc, "header_edges", record_option, around, model=around == 128)


@pytest.mark.parametrize("around", [128, 16384])
def test_header_edges_positions(enc, around):
    _check_positions(enc, "header_edges_positions", around, model=around == 128)


@pytest.mark.parametrize("record_option", K.RECORD_OPTIONS)
def test_first_blocks(enc, record_option):
    _check_postings(enc, "first_blocks", record_option)


@pytest.mark.parametrize("record_option", [K.WITH_FREQS, K.WITH_FREQS_AND_POSITIONS])
@pytest.mark.parametrize("avg", K.AVGS)
def test_block_max_ties(enc, avg, record_option):
    _check_postings(enc, "block_max_ties", avg, record_option)


@pytest.mark.parametrize("record_option", K.RECORD_OPTIONS)
@pytest.mark.parametrize("target", K.SCAN_TARGETS)
def test_scan_shapes(enc, target, record_option):
    _check_postings(enc, "scan_shapes", target, record_option, model=target <= 4097)


@pytest.mark.parametrize("target", K.SCAN_TARGETS)
def test_scan_shapes_positions(enc, target):
    _check_positions(enc, "scan_shapes_positions", target, model=target <= 4097)


def test_scan_257_partials_positions(enc):
    """More than 1 048 576 items: scan_top_kernel's carry loop goes round twice, and the term loops
    of the measure and write kernels stride (524 244 terms over at most 32 768 wavefronts)."""
    assert K.n_items_partials(_positions("scan_shapes_positions", K.SCAN_LARGE)[0][0])[1] == 257
    _check_positions(enc, "scan_shapes_positions", K.SCAN_LARGE, model=False)


def test_scan_257_partials_postings(enc):
    _check_postings(enc, "scan_shapes", K.SCAN_LARGE, K.WITH_FREQS_AND_POSITIONS, model=False)


# ------------------------------------------------------------------ device entry points
class _Device:
    """Inputs of one case on the device, and a poisoned output: GUARD | cap | GUARD bytes of 0xA5."""

    def __init__(self, case, cap):
        import torch

        self.torch = torch
        self.case = case
        self.positions = len(case) == 2
        cuda = torch.device("cuda", 0)
        up = lambda a, view: torch.from_numpy(np.ascontiguousarray(a).view(view)).to(cuda)
        self.h_ts = np.ascontiguousarray(case[0], np.uint64)
        self.n = len(self.h_ts) - 1
        self.d_ts = up(self.h_ts, np.int64)
        self.d_vals = up(case[1], np.int32)
        self.d_tfs = None if self.positions else up(case[2], np.int32)
        self.d_fn = None if self.positions or case[3] is None else up(case[3], np.uint8)
        self.cap = cap
        self.buf = torch.empty(GUARD + cap + GUARD, dtype=torch.uint8, device=cuda)
        self.d_ots = torch.zeros(self.n + 1, dtype=torch.int64, device=cuda)
        self.poison()

    def poison(self):
        self.buf.fill_(POISON)
        self.d_ots.fill_(-1)
        self.torch.cuda.synchronize()

    def run(self, enc, stream=None):
        """(return code, *out_len); the output is complete once this returns."""
        from tantivy_amd import binding as B

        L = B.lib()
        out_len = C.c_uint64(0xDEAD)
        d_out = self.buf.data_ptr() + GUARD
        assert d_out % 4 == 0
        hs = None if stream is None else C.c_void_p(stream.cuda_stream)
        if self.positions:
            rc = L.tq_encode_positions_device(enc.raw, self.n, self.h_ts.ctypes.data, self.d_ts.data_ptr(),
                                              self.d_vals.data_ptr(), d_out, self.cap,
                                              self.d_ots.data_ptr(), C.byref(out_len), hs)
        else:
            _, _, _, _, num_docs, avg, opt = self.case
            rc = L.tq_encode_postings_device(
                enc.raw, self.n, self.h_ts.ctypes.data, self.d_ts.data_ptr(), self.d_vals.data_ptr(),
                None if opt == K.BASIC else self.d_tfs.data_ptr(),
                None if self.d_fn is None else self.d_fn.data_ptr(), int(num_docs), C.c_float(avg),
                int(opt), d_out, self.cap, self.d_ots.data_ptr(), C.byref(out_len), hs)
        self.torch.cuda.synchronize()
        return rc, out_len.value

    def host(self):
        b = self.buf.cpu().numpy()
        return b[:GUARD], b[GUARD: GUARD + self.cap], b[GUARD + self.cap:], self.d_ots.cpu().numpy().view(np.uint64)


def _device_cases():
    out = [("width_matrix", d, opt) for d in (False, True) for opt in K.RECORD_OPTIONS]
    return out + [("position_widths", False), ("position_widths", True)]


def _cached(key):
    return (_positions if key[0] == "position_widths" else _postings)(*key)


@pytest.mark.parametrize("key", _device_cases(), ids=lambda k: "-".join(str(x) for x in k))
def test_device_entry_points_write_exactly_their_bytes(enc, key):
    """cap = the exact length, guards before and after: every byte of the body is written (the
    buffer starts as 0xA5, not as zeros), none outside; twice into the same buffer, then once on
    the caller's own stream."""
    case, want, want_ts = _cached(key)
    dev = _Device(case, int(want.size))
    for stream in (None, None, dev.torch.cuda.Stream()):
        dev.poison()
        rc, out_len = dev.run(enc, stream)
        assert rc == 0 and out_len == want.size
        before, body, after, ots = dev.host()
        assert (before == POISON).all() and (after == POISON).all()
        _expect(body, ots, want, want_ts, "stream %s" % (stream is not None))


@pytest.mark.parametrize("key", [("width_matrix", True, K.WITH_FREQS_AND_POSITIONS), ("position_widths", False)],
                         ids=["postings", "positions"])
def test_device_buffer_one_byte_too_small(enc, key):
    case, want, want_ts = _cached(key)
    dev = _Device(case, int(want.size) - 1)
    rc, out_len = dev.run(enc)
    assert rc != 0 and out_len == want.size
    assert (dev.buf.cpu().numpy() == POISON).all()  # not one byte has changed
    # and the encoder still works
    got, got_ts = _encode(enc, case)
    _expect(got, got_ts, want, want_ts)


# ------------------------------------------------------------------ one encoder, many calls
def test_one_encoder_many_calls(ta):
    """Grow-only scratch and staging: a call after a larger one must not see the earlier call's
    blk_meta / blk_tfsum / sizes / bytes."""
    from tantivy_amd import binding as B

    e = ta.Encoder(0)
    try:
        big = _positions("header_edges_positions", 16384)
        steps = [big, _postings("vint_edges", K.BASIC),
                 _postings("first_blocks", K.WITH_FREQS_AND_POSITIONS)]
        for case, want, want_ts in steps:
            _expect(*_encode(e, case), want, want_ts)
        body, ots = e.encode_postings(np.zeros(1, np.uint64), np.zeros(0, np.uint32), None, None, 0, 0.0, K.BASIC)
        assert body.size == 0 and ots.tolist() == [0]
        # five empty terms, values NULL
        ts = np.zeros(6, np.uint64)
        out = np.full(16, POISON, np.uint8)
        h_ots = np.full(6, 77, np.uint64)
        need = C.c_uint64(0xDEAD)
        B._check(B.lib().tq_encode_postings(e.raw, 5, ts.ctypes.data, None, None, None, 0, C.c_float(0.0),
                                            K.WITH_FREQS, out.ctypes.data, out.size, h_ots.ctypes.data,
                                            C.byref(need)))
        assert need.value == 0 and h_ots.tolist() == [0] * 6 and (out == POISON).all()
        want, want_ts = O.serialize_postings_batch(ts, np.zeros(0, np.uint32), None, None, 0, 0.0, K.WITH_FREQS)
        assert want.size == 0 and want_ts.tolist() == [0] * 6
        for case, want, want_ts in (_postings("width_matrix", True, K.WITH_FREQS), big):
            _expect(*_encode(e, case), want, want_ts)
    finally:
        e.close()


# ------------------------------------------------------------------ argument errors
def test_argument_errors_leave_the_encoder_usable(ta, enc):
    docs = np.arange(300, dtype=np.uint32)
    tfs = np.ones(300, np.uint32)
    good, want, want_ts = _postings("vint_edges", K.WITH_FREQS)
    calls = [
        lambda: enc.encode_postings(np.array([0, 200, 100], np.uint64), docs, tfs, None, 0, 0.0, K.WITH_FREQS),
        lambda: enc.encode_positions(np.array([0, 200, 100], np.uint64), docs),
        lambda: enc.encode_postings(np.array([5, 200], np.uint64), docs, tfs, None, 0, 0.0, K.WITH_FREQS),
        lambda: enc.encode_positions(np.array([5, 200], np.uint64), docs),
        lambda: enc.encode_postings(np.array([0, 200], np.uint64), docs, tfs, None, 0, 0.0, 3),
    ]
    for call in calls:
        with pytest.raises(ta.TantivyAmdError):
            call()
        _expect(*_encode(enc, good), want, want_ts)


def test_argument_errors_on_the_device_path(ta, enc):
    case, want, want_ts = _postings("vint_edges", K.WITH_FREQS)
    dev = _Device(case, int(want.size))
    ok_ts = dev.h_ts
    bad = ok_ts.copy()
    bad[3] = bad[5]  # term 3 now starts after term 4: term_starts decreases
    assert bad[4] < bad[3]
    dev.h_ts = bad
    rc, _ = dev.run(enc)
    assert rc != 0 and (dev.buf.cpu().numpy() == POISON).all()
    dev.h_ts = ok_ts
    dev.case = case[:6] + (3,)
    rc, _ = dev.run(enc)
    assert rc != 0 and (dev.buf.cpu().numpy() == POISON).all()
    dev.case = case
    rc, out_len = dev.run(enc)
    assert rc == 0 and out_len == want.size
    _, body, _, ots = dev.host()
    _expect(body, ots, want, want_ts)


# ------------------------------------------------------------------ the grid cap
# A child takes about as long as importing the package, creating a context and four small encodes
# (0.4 s measured on an MI355X, a few seconds on a busy machine); only a hung child reaches the limit.
CHILD_TIMEOUT_S = 120


def test_grid_cap_in_a_child_process():
    """TQ_ENC_WGS=1 and =3: the chunk loops of enc_measure_kernel / enc_write_kernel go round
    several times and there are more terms than wavefronts.  The cap is read once per process, so
    each value gets a fresh child, one after the other; a child that ends by a signal or at its
    time limit fails the test at once and no further child is started."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for wgs in ("1", "3"):
        env = dict(os.environ, TQ_ENC_WGS=wgs)
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "tests.encode_grid_child", "grid"]
        r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        assert r.returncode == 0, "TQ_ENC_WGS=%s: exit %d\n%s" % (wgs, r.returncode, r.stderr[-2000:])
