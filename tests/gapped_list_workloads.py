"""Workloads of the gapped mismatch list tests (CPU test, GPU test, CLI test) -- TEST INFRASTRUCTURE ONLY.

workload()    gap_workloads.workload with one more class: in every second planted deletion (classes D and E) the target's first
              base behind the deletion is substituted, so that the first aligned mismatch directly follows the deleted bases
              (MD 40^AC0T57).  gap_workloads.py itself is not edited.
hand_cases()  gap records written by hand over a text of its own -- no matcher and no rescue behind them: every read length,
              split, gap length, target mate and strand the list kernel takes another path at, placements at text position 0
              and on the text's last base, N bits inside deleted ranges and aligned segments, and the records that must give an
              empty list.  The contract of the stage on such a record is its geometry alone.
Both are functions of their arguments.
"""
from __future__ import annotations

import numpy as np

import gap_checker as gc
import gap_workloads as gw

LENGTHS = (25, 31, 32, 33, 63, 64, 65, 100, 320)
GAPS = (-16, -8, -1, 0, 1, 8, 16)
MIN_FLANK = 8
HAND_N = 30_000 + 13                      # no multiple of 32 or 64
N_REGION = (12_000, 18_000)               # where the text carries N bits


def workload(**kw):
    w = gw.workload(**kw)
    patl = w["patl"]
    turn = 0
    for p in w["plants"]:
        if p["cls"] not in "DE" or p["g"] <= 0:
            continue
        turn += 1
        if turn % 2:
            continue
        b = (w["b1"], w["b2"])[p["tm"]]
        at = p["split"] if p["tfwd"] else patl - 1 - p["split"]     # oriented offset `split`: the first base behind the deletion
        b.bases[int(b.offsets[p["i"]]) + at] ^= 2
        p["follows"] = True
    return w


def splits_of(l: int, g: int):
    d = max(-g, 0)
    if g == 0:
        return [0]
    want = {1, MIN_FLANK, 31, 32, 33, 64, l - MIN_FLANK, l - 1 - d}
    return sorted(j for j in want if 1 <= j and j + d <= l - 1)


def _record(pos, tm, inv, state, j, g, k, fileid=0):
    r = gc.empty_records(1)[0]
    r["pos"], r["fileid"], r["split"], r["gap"], r["k"], r["cost"] = pos, fileid, j, g, k, gc.cost_of(k, g, gc.default_params())
    r["tag"] = tm | (inv << 4) | (state << 5)
    return r


def hand_cases(seed=3, fileid=0):
    """{sym, frag_start, b1, b2, gaps, what: [str], fileid}"""
    rng = np.random.default_rng(seed)
    n = HAND_N
    sym = rng.integers(0, 4, size=n).astype(np.uint8)
    lo, hi = N_REGION
    sym[lo + np.nonzero(rng.random(hi - lo) < 0.03)[0]] = 4
    reads1, reads2, recs, what = [], [], [], []

    def add(l, g, j, tm, inv, pos, state=gc.UNIQUE, subs=2, k_off=0, file=fileid, note=""):
        """a read of l bases that follows the text at pos with gap g at split j, but for `subs` substitutions"""
        d, dele = max(-g, 0), max(g, 0)
        span = l + g
        src = np.where(sym > 3, 1, sym)                                  # (a read shows a base where the text has none)
        p = max(0, min(pos, n - span))                                   # the read's content is cut from inside the text whatever the record says
        o = np.concatenate([src[p:p + j], rng.integers(0, 4, size=d).astype(np.uint8), src[p + j + dele:p + span]]) if g else src[p:p + l].copy()
        o = np.resize(o, l) if o.shape[0] != l else o                    # (records that do not fit: any l bases)
        o = o.astype(np.uint8)
        k = 0
        for x in rng.choice(l, size=min(subs, l), replace=False):
            o[x] ^= 1 + int(rng.integers(0, 3))
            k += 0 if j <= x < j + d else 1
        read = gc.COMP[o[::-1]] if inv else o
        other = rng.integers(0, 4, size=30).astype(np.uint8)
        reads1.append(read if tm == 0 else other)
        reads2.append(other if tm == 0 else read)
        recs.append(_record(pos, tm, inv, state, j, g, max(0, min(15, k + k_off)), file))
        what.append(note or "L%d g%d j%d" % (l, g, j))

    turn = 0
    for l in LENGTHS:
        for g in GAPS:
            if l + g < 2 or (g < 0 and l - 1 + g < 1):
                continue
            for j in splits_of(l, g):
                tm, inv = turn & 1, (turn >> 1) & 1
                span = l + g
                where = turn % 7
                pos = 0 if where == 0 else n - span if where == 1 else int(rng.integers(lo, hi - span)) if where in (2, 3) else int(rng.integers(64, lo - span))
                add(l, g, j, tm, inv, pos, k_off=1 if turn % 11 == 5 else 0)
                turn += 1
    # N bits inside a deleted range and inside both aligned segments, on purpose
    for tm, inv in gw.COMBOS:
        pos = int(rng.integers(lo, hi - 200))
        sym[pos + 5], sym[pos + 41], sym[pos + 43], sym[pos + 90] = 4, 4, 4, 4
        add(100, 8, 40, tm, int(not inv), pos, note="N in the deletion and in both segments")
    # the records that must give an empty list
    ok = dict(l=100, g=2, j=40, tm=0, inv=0, pos=2000)
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
    return dict(sym=sym, frag_start=np.array([0, n], dtype=np.uint64), b1=gw.Batch(reads1), b2=gw.Batch(reads2), gaps=gaps, what=what, fileid=fileid)


EMPTY_NOTES = {"NoMatch": None, "NonUnique": None, "other file": "other_file", "pos + span = n + 1": "invalid", "ungapped, pos + L = n + 1": "invalid",
               "split 0 with a gap": "invalid", "split + d = L": "invalid", "split = L with a deletion": "invalid", "gap 17": "invalid", "gap -17": "invalid",
               "ungapped with a split": "invalid", "a read of 321 bases": "invalid", "a read of 321 bases with a gap": "invalid",
               "a position far behind the text": "invalid"}
