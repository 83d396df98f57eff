#!/usr/bin/env python
"""CPU model of what better STARTING thresholds could save the shared-intersection launch (no GPU): for the
headline batch (10 000 Zipf 2-term ANDs, 10M docs, k = 10) and each distinct query, the work of tq_ashare.hip's
stages under three sets of thresholds that stay fixed for the whole launch

  static     today's warm-up: the k-th best score among the matches in the first 0.2 % of the leader's blocks
             (leaders of fewer than 500 blocks have no warm-up task: threshold 0)
  champion   the k-th best score among the matches within the leader's 4 096 postings of highest tf/(tf+norm)
             (a "champion list" per leader, built once; the idea this tool was written to judge)
  final      the query's k-th best score (no launch can know more)

and counts, per set

  blocks / pairs   (leader, group of <= 32 distinct queries) blocks some query of the group still wants — block-max
                   bound of the leader + list 1's range maxima over the block's doc span — and (block, query) pairs
  past_bound       docs of those blocks whose leader tf/(tf+norm) passes the loosest bound of the block's
                   queries: each pays the 8-byte doc-matrix gather of stage A
  candidates       (doc, query) pairs that reach the scoring stage: in list 1, and leader score + list 1's range
                   maximum at the doc >= threshold
  collected        matches whose score reaches the threshold

Thresholds rise during a real launch: the static column is a ceiling of today's launch, the final one a floor (the
launch's own counters: 192 k blocks decoded, 2.3 M pairs, 8.7 M candidates, 2.3 M collected).  Membership in list 1 is
exact here; the kernel's stage F also lets the signature bits' "maybe" through, so its candidate counts are higher.
Last run (10 000 queries, 255 leaders, 3 877 distinct queries; 40 s):
              blocks        pairs   past_bound   candidates    collected
  static      200302      2405803     19907712     18182007     13311051
  champion    182400      2177140      5946546       559858        55959
  final       177633      2133744      3836681       459626        39527
-> better starting thresholds cannot remove blocks (89 % of them and of the pairs survive even the FINAL thresholds:
the launch is a scan of every leader), only scoring-stage work, which is under a tenth of the wave cycles.
Usage: python tools/sim/sim_ashare_thresholds.py [n_queries]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402

K, R, CHAMPIONS, WARM_PERMILLE, WARM_MIN_BLOCKS, GROUP = 10, 1024, 4096, 2, 500, 32


def main():
    n_q = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
    N = 10_000_000
    seg = O.synth_segment(N, n_terms=256)
    fn = np.frombuffer(seg.fieldnorm, dtype=np.uint8)
    table = np.array(O.fieldnorm_table(), dtype=np.float32)
    avg = np.float32(seg.total_num_tokens) / np.float32(N)
    cache = (np.float32(1.2) * (np.float32(0.25) + np.float32(0.75) * table / avg)).astype(np.float32)
    norm_doc = cache[fn]
    t0 = time.time()
    docs, tfa, rmax = [], [], []
    nr = (N + R - 1) // R
    for t in range(256):
        d, tf = O.decode_postings(seg, t)
        docs.append(d.astype(np.int64))
        a = np.zeros(N, dtype=np.uint8)
        a[d] = np.minimum(tf, 255)
        tfa.append(a)
        f = a.astype(np.float32)
        tfn = np.where(a > 0, f / (f + norm_doc), 0).astype(np.float32)
        rmax.append(np.pad(tfn, (0, nr * R - N)).reshape(nr, R).max(axis=1))
    print("decoded + range maxima in %.1f s" % (time.time() - t0), flush=True)
    dfs = [len(d) for d in docs]
    by_leader = {}
    for q in O.zipf_queries(n_q, 2, 256, seed=20260921):
        a, b = int(q[0]), int(q[1])
        l, s = (a, b) if dfs[a] <= dfs[b] else (b, a)
        if l != s:
            by_leader.setdefault(l, set()).add(s)
    print("%d leaders, %d distinct queries" % (len(by_leader), sum(len(v) for v in by_leader.values())))
    names = ("static", "champion", "final")
    tot = {n: dict(blocks=0, pairs=0, past_bound=0, candidates=0, collected=0) for n in names}
    for l, seconds in sorted(by_leader.items()):
        d0 = docs[l]
        f0 = tfa[l][d0].astype(np.float32)
        n0 = norm_doc[d0]
        tfn0 = f0 / (f0 + n0)
        n_blocks = (len(d0) + 127) // 128
        blk = np.arange(len(d0)) // 128
        blk_max = np.maximum.reduceat(tfn0, np.arange(0, len(d0), 128))
        first, last = d0[::128], d0[np.minimum(np.arange(n_blocks) * 128 + 127, len(d0) - 1)]
        warm = (n_blocks * WARM_PERMILLE // 1000) * 128 if n_blocks >= WARM_MIN_BLOCKS else 0
        champ = np.zeros(len(d0), dtype=bool)
        champ[np.argsort(-tfn0, kind="stable")[:CHAMPIONS]] = True
        seconds = sorted(seconds)
        for g0 in range(0, len(seconds), GROUP):
            need_blk = {n: np.full(n_blocks, np.inf, dtype=np.float32) for n in names}
            for s in seconds[g0:g0 + GROUP]:
                w = O.default_weights(seg, [l, s], O.MODE_AND)
                w0, w1 = np.float32(w[0].weight), np.float32(w[1].weight)
                tf1 = tfa[s][d0]
                m = tf1 > 0
                f1 = tf1.astype(np.float32)
                sc = np.where(m, w0 * tfn0 + w1 * (f1 / (f1 + n0)), np.float32(-1)).astype(np.float32)

                def kth(sel):
                    x = sc[sel & m]
                    return np.partition(x, -K)[-K] if len(x) >= K else np.float32(0)

                thr = {"static": kth(np.arange(len(d0)) < warm), "champion": kth(champ), "final": kth(np.ones(len(d0), dtype=bool))}
                r1 = w1 * rmax[s][d0 // R]                                   # list 1's bound at the doc
                r1_blk = w1 * np.maximum(rmax[s][first // R], rmax[s][last // R])  # ... over the block's span (<= two entries; wider spans: looser in the kernel)
                for n in names:
                    want = w0 * blk_max + r1_blk >= thr[n]
                    need = np.where(want, (thr[n] - r1_blk) / w0, np.inf).astype(np.float32)
                    need_blk[n] = np.minimum(need_blk[n], need)
                    tot[n]["pairs"] += int(want.sum())
                    tot[n]["candidates"] += int((m & want[blk] & (w0 * tfn0 + r1 >= thr[n])).sum())
                    tot[n]["collected"] += int((m & (sc >= thr[n])).sum())
            for n in names:
                wanted = np.isfinite(need_blk[n])
                tot[n]["blocks"] += int(wanted.sum())
                tot[n]["past_bound"] += int((wanted[blk] & (tfn0 >= need_blk[n][blk])).sum())
    print("%-10s %12s %12s %12s %12s %12s" % ("", "blocks", "pairs", "past_bound", "candidates", "collected"))
    for n in names:
        t = tot[n]
        print("%-10s %12d %12d %12d %12d %12d" % (n, t["blocks"], t["pairs"], t["past_bound"], t["candidates"], t["collected"]))
    print("%.1f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
