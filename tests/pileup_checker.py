"""The pileup restated in numpy -- TEST INFRASTRUCTURE ONLY (include/real_hip.h, "pileup"): depth, alt counts, sites and
statistics from records, reads and the genome's symbols.  It is fed the ORACLE's records and never calls the code under
test.  Everything is an integer."""
from __future__ import annotations

import numpy as np

UNIQUE = 1                          # REAL_HIP_PAIR_UNIQUE
SITE_DTYPE = np.dtype([("pos", "<u4"), ("depth", "<u4"), ("alt", "<u4", (4,)), ("ref", "<u4"), ("reserved", "<u4")])
COUNTERS = ("reads", "placed", "other_file", "invalid", "bases", "mismatches", "low_qual", "n_dropped")


class Pileup:
    """the accumulators of one genome file: sym = its symbols 0..4 (4 = N; the 2-bit text stores an N as 0)"""

    def __init__(self, sym, fileid: int = 0, min_qual: int = 0):
        self.sym = np.asarray(sym, dtype=np.uint8)
        self.n = int(self.sym.shape[0])
        self.ref = np.where(self.sym > 3, 0, self.sym).astype(np.int64)
        self.is_n = self.sym > 3
        self.fileid, self.min_qual = int(fileid), int(min_qual)
        self.depth = np.zeros(self.n, dtype=np.int64)
        self.alt = np.zeros((self.n, 4), dtype=np.int64)
        self.stats = {k: 0 for k in COUNTERS}

    def place(self, read, qual, p: int, inverted: bool):
        """one placement: the read's bases 0..3, its qualities (None: 30 each), the text position, the strand"""
        read = np.asarray(read, dtype=np.int64)
        L = int(read.shape[0])
        if p + L > self.n:
            self.stats["invalid"] += 1
            return
        q = np.full(L, 30, dtype=np.int64) if qual is None else np.asarray(qual, dtype=np.int64)
        if inverted:
            read, q = 3 - read[::-1], q[::-1]
        self.stats["placed"] += 1
        self.stats["bases"] += L
        self.depth[p:p + L] += 1
        x = np.arange(p, p + L)
        mis = read != self.ref[x]
        low = mis & (q < self.min_qual)
        on_n = mis & ~low & self.is_n[x]
        take = mis & ~low & ~on_n
        self.stats["low_qual"] += int(low.sum())
        self.stats["n_dropped"] += int(on_n.sum())
        self.stats["mismatches"] += int(take.sum())
        np.add.at(self.alt, (x[take], read[take]), 1)

    def _read(self, b, i):
        lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
        return b.bases[lo:hi], (None if b.qual is None else b.qual[lo:hi])

    def add(self, b, info):
        """single-end: b has bases / qual / offsets, info the 64-bit UniqueMatchInfo records"""
        info = np.asarray(info, dtype=np.uint64)
        state = (info >> np.uint64(61)).astype(np.int64)
        fileid = ((info >> np.uint64(35)) & np.uint64(63)).astype(np.int64)
        pos = (info & np.uint64((1 << 35) - 1)).astype(np.int64)
        self.stats["reads"] += int(info.shape[0])
        for i in np.nonzero((state == 1) | (state == 2))[0]:
            if fileid[i] != self.fileid:
                self.stats["other_file"] += 1
                continue
            self.place(*self._read(b, i), int(pos[i]), state[i] == 2)

    def add_pairs(self, b1, b2, pairs):
        """paired-end: mate 1 at pos1 on strand inverted1, mate 2 at pos2 on the other one, for the Unique records"""
        self.stats["reads"] += 2 * int(pairs.shape[0])
        for i in np.nonzero(pairs["state"] == UNIQUE)[0]:
            if int(pairs["fileid"][i]) != self.fileid:
                self.stats["other_file"] += 2
                continue
            inv1 = bool(pairs["inverted1"][i])
            self.place(*self._read(b1, i), int(pairs["pos1"][i]), inv1)
            self.place(*self._read(b2, i), int(pairs["pos2"][i]), not inv1)

    def sites(self):
        at = np.nonzero(self.alt.sum(axis=1) > 0)[0]
        s = np.zeros(at.shape[0], dtype=SITE_DTYPE)
        s["pos"], s["depth"], s["alt"], s["ref"] = at, self.depth[at], self.alt[at], self.ref[at]
        return s

    def finish_stats(self):
        """every field of real_hip_pileup_stats but launches and kernel_ms"""
        return dict(self.stats, covered=int((self.depth > 0).sum()), sites=int((self.alt.sum(axis=1) > 0).sum()),
                    max_depth=int(self.depth.max()) if self.n else 0)


# ---- what `real -pileup` / `-pileup_depth` write, from a finished checker pileup -----------------------------------
def _frag_of(frag_start, x):
    return int(np.searchsorted(np.asarray(frag_start, dtype=np.int64), x, side="right")) - 1


def pileup_lines(pu: Pileup, frag_start, frag_names):
    out = []
    fs = np.asarray(frag_start, dtype=np.int64)
    for s in pu.sites():
        f = _frag_of(fs, int(s["pos"]))
        out.append("%s\t%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % (frag_names[f], int(s["pos"]) - int(fs[f]) + 1, "ACGT"[int(s["ref"])], int(s["depth"]),
                                                     *[int(v) for v in s["alt"]]))
    return "".join(out)


def depth_lines(pu: Pileup, frag_start, frag_names):
    """maximal runs of equal non-zero depth that do not cross a fragment boundary: name, 0-based start, end, depth"""
    out = []
    fs = np.asarray(frag_start, dtype=np.int64)
    for f in range(len(fs) - 1):
        d = pu.depth[fs[f]:fs[f + 1]]
        if not d.shape[0]:
            continue
        cut = np.concatenate([[0], np.nonzero(d[1:] != d[:-1])[0] + 1, [d.shape[0]]])
        for a, e in zip(cut[:-1], cut[1:]):
            if d[a]:
                out.append("%s\t%d\t%d\t%d\n" % (frag_names[f], a, e, d[a]))
    return "".join(out)


def stderr_line(pu: Pileup, name: str):
    st = pu.finish_stats()
    return "pileup: file=%s placements=%d bases=%d covered=%d mean_depth=%.3f max_depth=%d sites=%d mismatches=%d low_qual=%d" % (
        name, st["placed"], st["bases"], st["covered"], st["bases"] / st["covered"] if st["covered"] else 0.0, st["max_depth"], st["sites"],
        st["mismatches"], st["low_qual"])
