"""The gapped placements in the pileup and the calls, restated in numpy -- TEST INFRASTRUCTURE ONLY (include/real_hip.h, "gapped
placements in the pileup and the calls").  pileup_checker.Pileup with gdepth and place_gapped, call_checker.Calls with the gapped
evidence.  It is fed the ORACLE's records (or records written by hand) and never calls the code under test.  Two formulations of
the aligned (oriented read offset, text position) pairs of one placement:
  aligned_by_pairs      the pairs listed one by one (gap_checker.aligned_pairs);
  aligned_by_diagonals  the two diagonals sliced: read [0, j) on text p + r, read [j + d, L) on text p + r + g.
Everything is an integer."""
from __future__ import annotations

import types

import numpy as np

import call_checker as ck
import gap_checker as gc
import gapped_list_checker as glc
import pileup_checker as pk

COUNTERS = ("records", "placed", "other_file", "invalid", "ungapped", "aligned_bases", "deleted", "inserted", "mismatches", "low_qual", "n_dropped")
CALL_COUNTERS = ("site_bases", "site_low_qual")


def aligned_by_pairs(l: int, p: int, g: int, j: int):
    """-> (oriented read offsets, text positions) as int64 arrays, in ascending text position"""
    al = gc.aligned_pairs(l, p, g, j)
    return np.array([a for a, _ in al], dtype=np.int64), np.array([x for _, x in al], dtype=np.int64)


def aligned_by_diagonals(l: int, p: int, g: int, j: int):
    if g == 0:
        r = np.arange(l, dtype=np.int64)
        return r, p + r
    d = max(-g, 0)
    r1, r2 = np.arange(0, j, dtype=np.int64), np.arange(j + d, l, dtype=np.int64)
    return np.concatenate([r1, r2]), np.concatenate([p + r1, p + r2 + g])


def _oriented(read, qual, inverted: bool):
    r = gc.oriented(read, inverted).astype(np.int64)
    q = np.full(r.shape[0], 30, dtype=np.int64) if qual is None else np.asarray(qual, dtype=np.int64)
    return r, (q[::-1] if inverted else q)


def _records(self, b1, b2, gaps):
    """the Unique records of this file that fit, by the rule of the gapped lists: (i, read, qual, p, g, j, inverted); the
    others are counted in self.gstats where the caller keeps those counters"""
    count = "records" in self.gstats
    if count:
        self.gstats["records"] += int(gaps.shape[0])
    pu = getattr(self, "pu", self)
    for i in range(int(gaps.shape[0])):
        rec = gaps[i]
        if int(gc.state_of(rec["tag"])) != gc.UNIQUE:
            continue
        if int(rec["fileid"]) != pu.fileid:
            if count:
                self.gstats["other_file"] += 1
            continue
        b = (b1, b2)[int(gc.target_of(rec["tag"]))]
        lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
        if not glc.fits(rec, hi - lo, pu.n):
            if count:
                self.gstats["invalid"] += 1
            continue
        yield i, b.bases[lo:hi], (None if b.qual is None else b.qual[lo:hi]), int(rec["pos"]), int(rec["gap"]), int(rec["split"]), bool(gc.inverted_of(rec["tag"]))


class GappedPileup(pk.Pileup):
    """pk.Pileup that also takes gapped placements: depth and alt hold everything, gdepth the gapped placements' share"""

    def __init__(self, sym, fileid: int = 0, min_qual: int = 0, aligned=aligned_by_pairs):
        super().__init__(sym, fileid, min_qual)
        self.gdepth = np.zeros(self.n, dtype=np.int64)
        self.gstats = dict.fromkeys(COUNTERS, 0)
        self.aligned = aligned
        self.increments = []                                             # per placed record: (text positions, bases) of its alt increments

    def place_gapped(self, read, qual, p: int, g: int, j: int, inverted: bool):
        """one fitting placement: the read's bases 0..3, its qualities (None: 30 each), position, gap, split, strand"""
        l = int(np.asarray(read).shape[0])
        r, q = _oriented(read, qual, inverted)
        ro, x = self.aligned(l, p, g, j)
        st = self.gstats
        st["placed"] += 1
        st["ungapped"] += g == 0
        st["aligned_bases"] += int(x.shape[0])
        st["deleted"] += max(g, 0)
        st["inserted"] += max(-g, 0)
        np.add.at(self.depth, x, 1)
        np.add.at(self.gdepth, x, 1)
        base, qq = r[ro], q[ro]
        mis = base != self.ref[x]
        low = mis & (qq < self.min_qual)
        on_n = mis & ~low & self.is_n[x]
        take = mis & ~low & ~on_n
        st["low_qual"] += int(low.sum())
        st["n_dropped"] += int(on_n.sum())
        st["mismatches"] += int(take.sum())
        np.add.at(self.alt, (x[take], base[take]), 1)
        self.increments.append((x[take], base[take]))

    def add_gapped(self, b1, b2, gaps):
        for _, read, qual, p, g, j, inv in _records(self, b1, b2, gaps):
            self.place_gapped(read, qual, p, g, j, inv)

    def ungapped_view(self):
        """what the indel calls stand on: this pileup with u = depth - gdepth for its depth (indel_checker.Indels reads sym, n,
        ref, fileid, min_qual and depth)"""
        return types.SimpleNamespace(sym=self.sym, n=self.n, ref=self.ref, fileid=self.fileid, min_qual=self.min_qual, depth=self.depth - self.gdepth)

    def gapped_stats(self):
        return {k: int(v) for k, v in self.gstats.items()}


class GappedCalls(ck.Calls):
    """ck.Calls over a finished GappedPileup, with the evidence of the gapped placements"""

    def __init__(self, pu: GappedPileup, aligned=aligned_by_pairs):
        super().__init__(pu)
        self.gstats = dict.fromkeys(CALL_COUNTERS, 0)
        self.aligned = aligned

    def place_gapped(self, read, qual, p: int, g: int, j: int, inverted: bool):
        l = int(np.asarray(read).shape[0])
        r, q = _oriented(read, qual, inverted)
        ro, x = self.aligned(l, p, g, j)
        s = self.slot[x]
        at = s >= 0
        good = at & (q[ro] >= self.pu.min_qual)
        self.gstats["site_low_qual"] += int((at & ~good).sum())
        self.gstats["site_bases"] += int(good.sum())
        np.add.at(self.cnt, (s[good], r[ro][good]), 1)
        np.add.at(self.qsum, (s[good], r[ro][good]), q[ro][good])

    def add_gapped(self, b1, b2, gaps):
        for _, read, qual, p, g, j, inv in _records(self, b1, b2, gaps):
            self.place_gapped(read, qual, p, g, j, inv)


def stderr_line(pu: GappedPileup, name: str) -> str:
    st = pu.gstats
    return "pileup gapped: file=%s placements=%d ungapped=%d aligned=%d deleted=%d inserted=%d mismatches=%d low_qual=%d" % (
        name, st["placed"], st["ungapped"], st["aligned_bases"], st["deleted"], st["inserted"], st["mismatches"], st["low_qual"])
