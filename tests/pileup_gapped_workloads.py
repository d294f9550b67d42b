"""Workloads of the tests of the gapped placements in the pileup and the calls (CPU test, GPU test) -- TEST INFRASTRUCTURE ONLY.

hand_cases()  gap records and pair records written by hand over a text of its own (100 kbp and 13 bases, no multiple of 32 or
              64) -- no matcher and no rescue behind them: the read lengths, gap lengths and splits the kernels take another
              path at, placements whose text position is 0 or 31 modulo 32, at position 0 and ending on the text's last base,
              deletions across a 32-position text word, both strands and both targets, N bits on aligned and on deleted
              positions, qualities on both sides of 20, several reads over one locus (sites of depth > 1 under first and second
              segments), and every record that must add nothing.  The pair records place ungapped mates over some of the same
              loci.
A function of its arguments.
"""
from __future__ import annotations

import numpy as np

import gap_checker as gc
import gap_workloads as gw
import indel_workloads as iw

HAND_N = 100_000 + 13
N_REGION = (40_000, 46_000)
LENGTHS = (25, 64, 65, 320)
GAPS = (-16, -1, 0, 1, 16)
EMPTY_NOTES = {"NoMatch": None, "NonUnique": None, "other file": "other_file", "pos + span = n + 1": "invalid", "ungapped, pos + L = n + 1": "invalid",
               "split 0 with a gap": "invalid", "split + d = L": "invalid", "split = L with a deletion": "invalid", "gap 17": "invalid", "gap -17": "invalid",
               "ungapped with a split": "invalid", "a read of 321 bases": "invalid", "a read of 321 bases with a gap": "invalid",
               "a position far behind the text": "invalid"}


def splits_of(l: int, g: int):
    d = max(-g, 0)
    if g == 0:
        return [0]
    return sorted(j for j in {1, 31, 32, 33, 64, l - 1 - d} if 1 <= j and j + d <= l - 1)


def hand_cases(seed=11, fileid=0):
    """{sym, frag_start, b1, b2, gaps, what: [str], pb1, pb2, pairs, fileid}"""
    rng = np.random.default_rng(seed)
    n = HAND_N
    sym = rng.integers(0, 4, size=n).astype(np.uint8)
    lo, hi = N_REGION
    sym[lo + np.nonzero(rng.random(hi - lo) < 0.03)[0]] = 4
    reads1, reads2, q1, q2, recs, what = [], [], [], [], [], []

    def add(l, g, j, tm, inv, pos, state=gc.UNIQUE, subs=3, file=fileid, note=""):
        """a read of l bases that follows the text at pos with gap g at split j, but for `subs` substitutions; qualities 5 .. 40"""
        d, dele = max(-g, 0), max(g, 0)
        span = l + g
        src = np.where(sym > 3, 1, sym)                                  # (a read shows a base where the text has none)
        p = max(0, min(pos, n - span))                                   # the read's content is cut from inside the text whatever the record says
        o = np.concatenate([src[p:p + j], rng.integers(0, 4, size=d).astype(np.uint8), src[p + j + dele:p + span]]) if g else src[p:p + l].copy()
        o = np.resize(o, l).astype(np.uint8)                             # (records that do not fit: any l bases)
        for x in rng.choice(l, size=min(subs, l), replace=False):
            o[x] ^= 1 + int(rng.integers(0, 3))
        qo = rng.integers(5, 41, size=l).astype(np.uint8)
        read, qr = (gc.COMP[o[::-1]], qo[::-1].copy()) if inv else (o, qo)
        other, qother = rng.integers(0, 4, size=30).astype(np.uint8), np.full(30, 35, dtype=np.uint8)
        reads1.append(read if tm == 0 else other)
        reads2.append(other if tm == 0 else read)
        q1.append(qr if tm == 0 else qother)
        q2.append(qother if tm == 0 else qr)
        r = gc.empty_records(1)[0]
        r["pos"], r["fileid"], r["split"], r["gap"], r["k"], r["cost"] = pos & 0xffffffff, file, j, g, 0, 7
        r["tag"] = tm | (inv << 4) | (state << 5)
        recs.append(r)
        what.append(note or "L%d g%d j%d p%d" % (l, g, j, pos))

    # every length, gap and split; the placement's text position 0 or 31 modulo 32 in turn, then position 0, the text's end, the N region
    turn = 0
    for l in LENGTHS:
        for g in GAPS:
            for j in splits_of(l, g):
                span = l + g
                for where in range(5):
                    tm, inv = turn & 1, (turn >> 1) & 1
                    if where == 0:
                        pos = 32 * int(rng.integers(10, 1_000))
                    elif where == 1:
                        pos = 32 * int(rng.integers(10, 1_000)) + 31
                    elif where == 2:
                        pos = int(rng.integers(lo, hi - span))
                    elif where == 3:
                        pos = 0 if (turn // 5) % 2 == 0 else n - span
                    else:
                        pos = 50_000 + int(rng.integers(0, 700))            # a crowded stretch: sites of depth > 1 under both segments
                    add(l, g, j, tm, inv, pos)
                    turn += 1
    # deletions across a 32-position text word: the deleted range [p + j, p + j + g) holds a multiple of 32
    for k, (tm, inv) in enumerate(gw.COMBOS * 2):
        g = (2, 16)[k & 1]
        for j in (31, 40):
            pos = 32 * (2_000 + 3 * k) + (32 - j % 32) - 1                   # p + j = 31 modulo 32
            add(100, g, j, tm, int(not inv), pos, note="a deletion across a text word")
    # N bits on deleted and on aligned positions, on purpose
    for tm, inv in gw.COMBOS:
        pos = int(rng.integers(lo, hi - 200))
        sym[pos + 5], sym[pos + 41], sym[pos + 43], sym[pos + 90] = 4, 4, 4, 4
        add(100, 8, 40, tm, int(not inv), pos, subs=12, note="N in the deletion and in both segments")
    # the records that must add nothing
    ok = dict(l=100, g=2, j=40, tm=0, inv=0, pos=2_000)
    add(**ok, state=gc.NOMATCH, note="NoMatch")
    add(**ok, state=gc.NONUNIQUE, note="NonUnique")
    add(**dict(ok, tm=1), file=fileid + 1, note="other file")
    add(**dict(ok, pos=n + 1 - 102), note="pos + span = n + 1")
    add(**dict(ok, g=0, j=0, pos=n + 1 - 100, inv=1), note="ungapped, pos + L = n + 1")
    add(**dict(ok, j=0), note="split 0 with a gap")
    add(**dict(ok, g=-3, j=97, tm=1), note="split + d = L")
    add(**dict(ok, g=3, j=100), note="split = L with a deletion")
    add(**dict(ok, g=17), note="gap 17")
    add(**dict(ok, g=-17, inv=1), note="gap -17")
    add(**dict(ok, g=0, j=5), note="ungapped with a split")
    add(**dict(ok, l=321, g=0, j=0, tm=1), note="a read of 321 bases")
    add(**dict(ok, l=321, g=1, j=40), note="a read of 321 bases with a gap")
    add(**dict(ok, pos=0xFFFFFF00), note="a position far behind the text")
    add(**ok, note="a fitting record behind them")
    gaps = np.array(recs, dtype=gc.REC_DTYPE)
    # the pair records: ungapped mates with substitutions over the crowded stretch and over the first kilobases
    src = np.where(sym > 3, 1, sym).astype(np.uint8)
    pr1, pr2, pq1, pq2, prec = [], [], [], [], []
    for k in range(150):
        p1 = (50_000 if k % 3 else 320) + int(rng.integers(0, 800))
        p2 = p1 + 150
        r = np.zeros(1, dtype=iw.PAIR_DTYPE)[0]
        r["pos1"], r["pos2"], r["fileid"], r["inverted1"], r["state"] = p1, p2, fileid, k & 1, 1
        a, b = src[p1:p1 + 100].copy(), src[p2:p2 + 100].copy()
        a[int(rng.integers(0, 100))] ^= 2
        b[int(rng.integers(0, 100))] ^= 1
        pr1.append(gc.COMP[a[::-1]] if k & 1 else a)
        pr2.append(b if k & 1 else gc.COMP[b[::-1]])
        pq1.append(rng.integers(5, 41, size=100).astype(np.uint8))
        pq2.append(rng.integers(5, 41, size=100).astype(np.uint8))
        prec.append(r)
    return dict(sym=sym, frag_start=np.array([0, n], dtype=np.uint64), b1=iw.Batch(reads1, q1), b2=iw.Batch(reads2, q2), gaps=gaps, what=what,
                pb1=iw.Batch(pr1, pq1), pb2=iw.Batch(pr2, pq2), pairs=np.array(prec, dtype=iw.PAIR_DTYPE), fileid=fileid)
