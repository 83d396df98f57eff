"""Child process of test_gpu_encode_edges.py: encodes one case with the grid cap the parent put
into TQ_ENC_WGS (read once per process, hence a process of its own), for all three record options
and the positions file, and compares the bytes with the oracle.  Exit status 0 = equal; 1 = a
difference, with the first differing offsets on stderr.

    python -m tests.encode_grid_child grid"""
import sys

import numpy as np

from oracle import oracle as O
from tests import encode_cases as K


def grid_case(record_option):
    """About 700 full blocks over 40 terms: with TQ_ENC_WGS=1 (4 wavefronts of 32 blocks a trip)
    the block loops go round five or six times and the term loops ten times."""
    rng = np.random.default_rng(4900)
    num_docs = 200_000
    doc_lists, tf_lists = [], []
    for t in range(40):
        n = 128 * int(rng.integers(5, 31)) + int(rng.integers(0, 128))
        doc_lists.append(np.sort(rng.choice(num_docs, size=n, replace=False)))
        tf = rng.integers(1, 13, size=n)
        tf[int(rng.integers(0, n))] = 300 + t
        tf_lists.append(tf)
    ts, docs, tfs = K._assemble(doc_lists, tf_lists)
    fn = rng.integers(0, 256, size=num_docs).astype(np.uint8)
    return ts, docs, tfs, fn, num_docs, 37.25, record_option


def grid_case_positions():
    ts, _, tfs, _, _, _, _ = grid_case(K.BASIC)
    rng = np.random.default_rng(4901)
    deltas = rng.integers(0, 60, size=int(ts[-1])).astype(np.uint32)
    deltas[::97] = tfs[::97] << 12
    return ts, deltas


def main(argv):
    if argv[1:] != ["grid"]:
        print("usage: python -m tests.encode_grid_child grid", file=sys.stderr)
        return 2
    import tantivy_amd

    enc = tantivy_amd.Encoder(0)
    bad = 0
    try:
        for opt in K.RECORD_OPTIONS:
            case = grid_case(opt)
            want, want_ts = O.serialize_postings_batch(*case)
            got, got_ts = enc.encode_postings(case[0], case[1], None if opt == K.BASIC else case[2],
                                              *case[3:])
            for what, g, w in (("bytes", got, want), ("term starts", got_ts, want_ts)):
                diff = K.first_diff(g, w)
                if diff:
                    print("record option %d, %s: %s" % (opt, what, diff), file=sys.stderr)
                    bad = 1
        case = grid_case_positions()
        want, want_ts = O.serialize_positions_batch(*case)
        got, got_ts = enc.encode_positions(*case)
        for what, g, w in (("bytes", got, want), ("term starts", got_ts, want_ts)):
            diff = K.first_diff(g, w)
            if diff:
                print("positions, %s: %s" % (what, diff), file=sys.stderr)
                bad = 1
    finally:
        enc.close()
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv))
