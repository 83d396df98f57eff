"""The host format walker (tq_term_walk.cpp: host_walk_term) without a GPU: tools/planbench/walk_check.cpp walks every
term of segments written by the oracle's serializers and prints what the walk leaves in the term's blob — block records,
tails, coarse table — which is compared with the lists the segments were built from; malformed bytes are reported as
TQ_ERR_FORMAT."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import random_postings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TQ_ERR_FORMAT = 3
MAX_DOC = 20_000
# list lengths around the 128-posting block: one vint block, a full block with and without a tail, two and three blocks
DFS = [1, 127, 128, 129, 255, 256, 257, 3 * 128 + 1]


@pytest.fixture(scope="module")
def walk_check(tmp_path_factory):
    from tantivy_amd import build as B

    B.build()
    out = tmp_path_factory.mktemp("walk") / "walk_check"
    obj = str(out) + ".o"
    src = os.path.join(ROOT, "tools", "planbench", "walk_check.cpp")
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "-Wno-unused-function", "-fPIC", "-c", src, "-o", obj],
                          cwd=str(out.parent))
    objs = [os.path.join(B.OBJ_DIR, os.path.basename(s) + ".o") for s in B.SOURCES if os.sep + "csrc" + os.sep in s]
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-o", str(out), obj] + objs + ["-ldl", "-lpthread"],
                          cwd=str(out.parent))
    return str(out)


def run_walk(walk_check, tmp_path, seg, infos=None):
    """-> per term: {"ok": ..., "n_blocks", "last_doc", "n_positions", "shift", "rec": [[4 u32]], "tail_docs", "tail_tfs",
    "coarse"} or {"ok": False, "code", "message"}"""
    idx, pos, terms = tmp_path / "idx", tmp_path / "pos", tmp_path / "terms"
    seg.idx[: seg.idx_len].tofile(str(idx))
    if seg.pos_len:
        seg.pos[: seg.pos_len].tofile(str(pos))
    if infos is None:
        infos = [(t.postings_start, t.postings_end - t.postings_start, t.positions_start, t.positions_end - t.positions_start,
                  t.doc_freq) for t in seg.terms]
    terms.write_text("".join("%d %d %d %d %d\n" % i for i in infos))
    r = subprocess.run([walk_check, str(idx), str(pos) if seg.pos_len else "-", str(terms), str(seg.record_option),
                        str(seg.max_doc)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr + r.stdout
    out = []
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] == "term" and f[2] == "ok":
            out.append({"ok": True, "rec": [], **{f[i]: int(f[i + 1]) for i in range(3, len(f), 2)}})
        elif f[0] == "term":
            out.append({"ok": False, "code": int(f[3]), "message": " ".join(f[4:])})
        elif f[0] == "rec":
            out[-1]["rec"].append([int(x) for x in f[1:]])
        else:
            out[-1][f[0]] = [int(x) for x in f[1:]]
    assert len(out) == len(infos), r.stdout[-2000:]
    return out


def shaped_lists(rng, record_option):
    """The lists of DFS, one whose last doc is max_doc - 1 and, with positions, two lists whose positions number exactly
    2 * 128 (no vint tail in the positions stream) and 2 * 128 + 5."""
    max_tf = 1 if record_option == O.BASIC else 6
    lists = [random_postings(rng, MAX_DOC, df, max_tf=max_tf) for df in DFS]
    last = random_postings(rng, MAX_DOC - 1, 129, max_tf=max_tf)
    lists.append(last + [(MAX_DOC - 1, 1)])
    if record_option == O.WITH_FREQS_AND_POSITIONS:
        docs = sorted(rng.choice(MAX_DOC, size=64, replace=False).tolist())
        lists.append([(d, 4) for d in docs])                       # 256 positions
        lists.append([(d, 4) for d in docs[:63]] + [(docs[63], 9)])  # 261 positions
    return lists


@pytest.mark.parametrize("record_option", [O.BASIC, O.WITH_FREQS, O.WITH_FREQS_AND_POSITIONS])
def test_walk_unrolls_every_list_shape(walk_check, tmp_path, record_option):
    rng = np.random.default_rng(11 + record_option)
    lists = shaped_lists(rng, record_option)
    with_pos = record_option == O.WITH_FREQS_AND_POSITIONS
    positions = [[sorted(rng.choice(1000, size=tf, replace=False).tolist()) for _, tf in pl] for pl in lists] if with_pos else None
    seg = O.build_segment(MAX_DOC, lists, rng.integers(1, 50, size=MAX_DOC).tolist(), record_option=record_option,
                          positions=positions)
    if with_pos:
        assert [sum(tf for _, tf in pl) for pl in lists[-2:]] == [256, 261]
    walked = run_walk(walk_check, tmp_path, seg)
    for pl, w in zip(lists, walked):
        assert w["ok"], w
        docs, tfs = [d for d, _ in pl], [tf for _, tf in pl]
        df, n_full, n_tail = len(pl), len(pl) // 128, len(pl) % 128
        n_blocks = n_full + (1 if n_tail else 0)
        assert w["n_blocks"] == n_blocks and len(w["rec"]) == n_blocks
        for i in range(n_full):
            assert w["rec"][i][0] == docs[128 * i + 127], (df, i)
        if n_tail:
            assert w["rec"][n_full][0] == docs[-1]
        assert w["tail_docs"] == docs[128 * n_full:]
        assert w["tail_tfs"] == tfs[128 * n_full:]
        assert w["last_doc"] == docs[-1]
        assert w["n_positions"] == (sum(tfs) if with_pos else 0)
        if with_pos:  # positions before each block
            assert [r[3] for r in w["rec"]] == [sum(tfs[:128 * i]) for i in range(n_blocks)]
        # the coarse table: the smallest shift from 7 that leaves at most two buckets per block (+ 2), coarse[b] = the first
        # block whose last doc >= b << shift, one entry past the last bucket as the sentinel
        shift = 7
        while ((MAX_DOC - 1) >> shift) + 1 > 2 * n_blocks + 2:
            shift += 1
        assert w["shift"] == shift
        n_buckets = ((MAX_DOC - 1) >> shift) + 1
        block_last = [r[0] for r in w["rec"]]
        want = [next((j for j, ld in enumerate(block_last) if ld >= (b << shift)), n_blocks) for b in range(n_buckets + 1)]
        assert w["coarse"] == want
        assert w["coarse"][-1] == n_blocks
        # payload offsets of the bit-packed blocks: from 0, each 16 * (doc_bits + tf_bits) behind the one before
        offs, want_off = [r[2] for r in w["rec"][:n_full]], 0
        for i in range(n_full):
            doc_bits, tf_bits = w["rec"][i][1] & 0x1F, (w["rec"][i][1] >> 8) & 0xFF
            assert offs[i] == want_off, (df, i)
            want_off += 16 * (doc_bits + tf_bits)
        assert offs == sorted(set(offs))  # strictly increasing


def test_walk_reports_malformed_lists(walk_check, tmp_path):
    # the corrupted skip entry of test_device_side_prepare_reports_corrupt_lists (tests/test_gpu_round2.py)
    rng = np.random.default_rng(5)
    seg = O.build_segment(50_000, [random_postings(rng, 50_000, 3000, max_tf=5)], rng.integers(1, 50, size=50_000).tolist())
    (w,) = run_walk(walk_check, tmp_path, seg)
    assert w["ok"] and w["n_blocks"] == 24
    bad = O.Segment(seg.max_doc, seg.record_option, seg.idx[: seg.idx_len].copy(), np.zeros(0, np.uint8),
                    seg.fieldnorm, seg.terms, seg.total_num_tokens)
    bad.idx[8 + 3 + 8 * 5:8 + 3 + 8 * 5 + 4] = 0  # last_doc of skip entry 5 := 0 (not increasing)
    (w,) = run_walk(walk_check, tmp_path, bad)
    assert not w["ok"] and w["code"] == TQ_ERR_FORMAT and "not increasing" in w["message"], w


def test_walk_reports_positions_range_outside_the_pos_file(walk_check, tmp_path):
    rng = np.random.default_rng(6)
    pl = random_postings(rng, MAX_DOC, 200, max_tf=3)
    seg = O.build_segment(MAX_DOC, [pl], rng.integers(1, 50, size=MAX_DOC).tolist(), record_option=O.WITH_FREQS_AND_POSITIONS,
                          positions=[[list(range(tf)) for _, tf in pl]])
    t = seg.terms[0]
    plen = t.postings_end - t.postings_start
    good = (t.postings_start, plen, t.positions_start, t.positions_end - t.positions_start, t.doc_freq)
    past = (t.postings_start, plen, seg.pos_len - 4, 16, t.doc_freq)
    beyond = (t.postings_start, plen, seg.pos_len + 1, 0, t.doc_freq)
    ok, w1, w2 = run_walk(walk_check, tmp_path, seg, [good, past, beyond])
    assert ok["ok"] and ok["n_positions"] == sum(tf for _, tf in pl)
    for w in (w1, w2):
        assert not w["ok"] and w["code"] == TQ_ERR_FORMAT and "pos file" in w["message"], w
