"""The checker of the anchored gap placement tests -- TEST INFRASTRUCTURE ONLY.

A numpy statement of the semantics in include/real_hip.h ("anchored gap placement") over the reads, their final info words,
the hit lists of the sub-read batch S(b, A) and the text.  It never calls the code under test and imports nothing of the
product.  The candidates of a window are gap_checker's (cumsum_candidates / brute_candidates, cost_of, split_range); the anchor
geometry, the union over the anchors, best / second and the merge M are this file's own.  Two formulations of the union:
  flat   every candidate of every anchor into one SET of rows, sorted;
  fold   anchor by anchor: the smallest key so far and the smallest cost of every examined start (v, p), merged.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import gap_checker as gc

NOMATCH, UNIQUE, NONUNIQUE, NONE = gc.NOMATCH, gc.UNIQUE, gc.NONUNIQUE, gc.NONE
MAX_PATL, ANCHORS_MAX = gc.MAX_PATL, 64
COUNTERS = ("reads", "eligible", "skipped", "crowded", "unanchored", "anchors", "invalid_anchors", "positions", "placed", "unique", "gapped")
AnchorParams = namedtuple("AnchorParams", "anchor_len max_anchors")
HIT_DTYPE = np.dtype([("read", "<u4"), ("pos", "<u4"), ("score", "<f4"), ("frag", "<u2"), ("k", "u1"), ("inverted", "u1")])
assert HIT_DTYPE.itemsize == 16


class SubBatch:
    """S(b, A): sub-read 2i is the first A bases of read i, sub-read 2i + 1 its last A; a read shorter than A gives two
    sub-reads of symbol 4, which no matcher places (the stage skips such a read)"""
    def __init__(self, b, a):
        n = int(b.offsets.shape[0]) - 1
        self.bases = np.full(2 * n * a, 4, dtype=np.uint8)
        self.qual = np.full(2 * n * a, 30, dtype=np.uint8)
        for i in range(n):
            lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
            if hi - lo < a:
                continue
            for e, s in ((0, lo), (1, hi - a)):
                self.bases[(2 * i + e) * a:(2 * i + e + 1) * a] = b.bases[s:s + a]
                if b.qual is not None:
                    self.qual[(2 * i + e) * a:(2 * i + e + 1) * a] = b.qual[s:s + a]
        self.offsets = (np.arange(2 * n + 1, dtype=np.uint64) * np.uint64(a)).astype(np.uint64)
        self.patl = a

    @property
    def n_reads(self):
        return int(self.offsets.shape[0]) - 1


def eligible(info, i):
    return info is None or (int(info[i]) >> 61) == 0


def anchor_diagonal(q, e, v, l, a):
    """the start of the oriented read's ungapped diagonal that a hit of sub-read e at q on strand v names"""
    return q if e == v else q - (l - a)


def anchor_valid(t, q, f, a):
    return f < len(t.frag_start) - 1 and t.frag_start[f] <= q and q + a <= t.frag_start[f + 1]


def anchor_window(c, max_gap, fs, fe):
    first, last = max(c - max_gap, fs), min(c + max_gap, fe - 1)
    return (first, last) if first <= last else None


def anchors_of(t, hits, hoff, i, l, a):
    """the hits of read i's two sub-reads as (valid, v, f, c)"""
    out = []
    for e in (0, 1):
        for x in range(int(hoff[2 * i + e]), int(hoff[2 * i + e + 1])):
            q, f, v = int(hits["pos"][x]), int(hits["frag"][x]), 1 if int(hits["inverted"][x]) else 0
            out.append((anchor_valid(t, q, f, a), v, f, anchor_diagonal(q, e, v, l, a)))
    return out


def window_rows(t, read, v, f, c, prm, candidates):
    """(examined starts, rows (cost, |g|, p, v, g, j, k, f)) of one valid anchor"""
    fs, fe = t.frag_start[f], t.frag_start[f + 1]
    w = anchor_window(c, prm.max_gap, fs, fe)
    if w is None:
        return 0, []
    rows = candidates(t, gc.oriented(read, v), w[0], w[1], fs, fe, prm)
    return w[1] - w[0] + 1, [(cost, ag, p, v, g, j, k, f) for cost, ag, p, g, j, k in rows]


def best_second_flat(per_anchor, prm):
    rows = sorted(set(r for rows in per_anchor for r in rows))
    if not rows:
        return None, NONE
    b = rows[0]
    others = [r[0] for r in rows if r[3] != b[3] or abs(r[2] - b[2]) > prm.max_gap]
    return b, (min(others) if others else NONE)


def best_second_fold(per_anchor, prm):
    best, starts = None, {}
    for rows in per_anchor:
        for r in rows:
            if best is None or r[:6] < best[:6]:
                best = r
            key = (r[3], r[2])
            starts[key] = min(starts.get(key, NONE), r[0])
    if best is None:
        return None, NONE
    second = NONE
    for (v, p), cost in starts.items():
        if v != best[3] or abs(p - best[2]) > prm.max_gap:
            second = min(second, cost)
    return best, second


def record_of(best, second, prm, fileid):
    rec = gc.empty_records(1)[0]
    if best is None:
        return rec
    cost, _, p, v, g, j, k, f = best
    state = NONUNIQUE if second != NONE and second <= cost + prm.margin else UNIQUE
    rec["pos"], rec["frag"], rec["fileid"], rec["split"], rec["gap"], rec["k"], rec["cost"], rec["second"] = p, f, fileid, j, g, k, cost, second
    rec["tag"] = (v << 4) | (state << 5)
    return rec


def merge_key(r):
    g = int(r["gap"])
    return (int(r["cost"]), abs(g), int(r["fileid"]), int(r["pos"]), int(gc.inverted_of(r["tag"])), g, int(r["split"]))


def merge(a, b, max_gap, margin):
    """M of the header: two records of one read into one"""
    if int(gc.state_of(a["tag"])) == NOMATCH:
        a, b = b, a
    if int(gc.state_of(b["tag"])) == NOMATCH:
        return a.copy()
    w, l = (a, b) if merge_key(a) <= merge_key(b) else (b, a)
    same = int(w["fileid"]) == int(l["fileid"]) and int(gc.inverted_of(w["tag"])) == int(gc.inverted_of(l["tag"])) and \
        abs(int(w["pos"]) - int(l["pos"])) <= max_gap
    second = min(int(w["second"]), int(l["second"]), NONE if same else int(l["cost"]))
    out = w.copy()
    state = NONUNIQUE if second != NONE and second <= int(w["cost"]) + margin else UNIQUE
    out["second"] = second
    out["tag"] = (int(gc.inverted_of(w["tag"])) << 4) | (state << 5)
    return out


def check_anchor(t, b, info, hits, hoff, prm, ap, out=None, candidates=gc.cumsum_candidates, union=best_second_flat):
    """(records, counters) of one call on the resident file t; out: the records to fold into (fresh = 0), None: fresh"""
    n = int(b.offsets.shape[0]) - 1
    a_len = ap.anchor_len
    fresh = out is None
    out = gc.empty_records(n) if fresh else out.copy()
    ctr = dict.fromkeys(COUNTERS, 0)
    ctr["reads"] = n
    for i in range(n):
        if not eligible(info, i):
            continue
        ctr["eligible"] += 1
        read = b.bases[int(b.offsets[i]):int(b.offsets[i + 1])]
        l = int(read.shape[0])
        if (read > 3).any() or l > MAX_PATL or l < 2 * prm.min_flank + prm.max_gap + 1 or l < a_len:
            ctr["skipped"] += 1
            continue
        nh = int(hoff[2 * i + 2]) - int(hoff[2 * i])
        if nh > ap.max_anchors:
            ctr["crowded"] += 1
            continue
        if nh == 0:
            ctr["unanchored"] += 1
            continue
        per_anchor = []
        for valid, v, f, c in anchors_of(t, hits, hoff, i, l, a_len):
            if not valid:
                ctr["invalid_anchors"] += 1
                continue
            ctr["anchors"] += 1
            npos, rows = window_rows(t, read, v, f, c, prm, candidates)
            ctr["positions"] += npos
            per_anchor.append(rows)
        best, second = union(per_anchor, prm)
        r = record_of(best, second, prm, t.fileid)
        st = int(gc.state_of(r["tag"]))
        ctr["placed"] += st != NOMATCH
        ctr["unique"] += st == UNIQUE
        ctr["gapped"] += st != NOMATCH and int(r["gap"]) != 0
        if st != NOMATCH:
            out[i] = r if fresh else merge(out[i], r, prm.max_gap, prm.margin)
    return out, ctr


assert_records_equal = gc.assert_records_equal
