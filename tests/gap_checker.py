"""The checker of the gap rescue tests -- TEST INFRASTRUCTURE ONLY.

A numpy statement of the semantics in include/real_hip.h ("gap rescue") over the reads, the final records and the text.  It
never calls the code under test and imports nothing of the product.  Two formulations of the candidate set:
  cumsum_candidates  every (p, g, j) of a window at once, from cumulative sums of the diagonals' mismatch vectors;
  brute_candidates   one alignment at a time: the list of (read offset, text position) pairs is built explicitly and the
                     bases are compared one by one (small windows only).
The record is built by sorting the keys (cost, |g|, p, g, j).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

NOMATCH, UNIQUE, NONUNIQUE = 0, 1, 2
MAX_PATL, MAX_INSERT, GAP_MAX, NONE = 320, 4096, 16, 0xFFFF
REC_DTYPE = np.dtype([("pos", "<u4"), ("frag", "<u2"), ("fileid", "u1"), ("tag", "u1"), ("split", "<u2"), ("gap", "i1"), ("k", "u1"),
                      ("cost", "<u2"), ("second", "<u2")])
assert REC_DTYPE.itemsize == 16
COUNTERS = ("fragments", "eligible", "other_file", "skipped", "positions", "placed", "unique", "gapped")
COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)

Params = namedtuple("Params", "max_gap min_flank cost_mismatch cost_open cost_extend max_cost margin")


def default_params(totalkmax=3, max_gap=8, min_flank=8, margin=0, max_cost=None):
    """the command line's: costs 4 / 6 / 1, max_cost = 4 e + 6 + G"""
    return Params(max_gap, min_flank, 4, 6, 1, 4 * totalkmax + 6 + max_gap if max_cost is None else max_cost, margin)


def state_of(tag):
    return (np.asarray(tag) >> 5) & 3


def inverted_of(tag):
    return (np.asarray(tag) >> 4) & 1


def target_of(tag):
    return np.asarray(tag) & 1


def empty_records(n):
    r = np.zeros(n, dtype=REC_DTYPE)
    r["second"] = NONE
    return r


def cost_of(k, g, prm):
    return prm.cost_mismatch * k + (prm.cost_open + prm.cost_extend * abs(g) if g else 0)


def window(a, inv, la, l, min_ins, max_ins, max_gap, fs, fe):
    """the examined starts [first, last] of a target of l bases beside an anchor at a on strand inv, or None"""
    if not inv:
        lo, hi = max(a, a + la - l, a + min_ins - l), a + max_ins - l
    else:
        lo, hi = a + la - max_ins, min(a, a + la - l, a + la - min_ins)
    if lo > hi:
        return None
    first, last = max(lo - max_gap, fs), min(hi + max_gap, fe - 1)
    return (first, last) if first <= last else None


def split_range(l, g, prm):
    """the allowed split points of gap g, inclusive"""
    return (0, 0) if g == 0 else (prm.min_flank, l - prm.min_flank - max(0, -g))


def span_of(l, g):
    return l + g


class Text:
    """a genome file: symbols 0..4, fragment starts, the N prefix sums"""
    def __init__(self, sym, frag_start, fileid=0):
        self.sym = np.asarray(sym, dtype=np.uint8)
        self.frag_start = [int(x) for x in frag_start]
        self.fileid = int(fileid)
        self.n = int(self.sym.shape[0])
        self.ncum = np.concatenate([[0], np.cumsum(self.sym > 3)]).astype(np.int64)


def cumsum_candidates(t: Text, r, first, last, fs, fe, prm):
    """every candidate of the window as a row (cost, |g|, p, g, j, k)"""
    l, gmax, m = int(r.shape[0]), prm.max_gap, prm.min_flank
    q0 = first - gmax
    nq = last + gmax - q0 + 1
    idx = q0 + np.arange(nq, dtype=np.int64)[:, None] + np.arange(l, dtype=np.int64)[None, :]
    inside = (idx >= 0) & (idx < t.n)
    txt = np.where(inside, t.sym[np.clip(idx, 0, t.n - 1)], 5)          # (bases outside the text match nothing; no valid span holds one)
    cum = np.zeros((nq, l + 1), dtype=np.int64)
    cum[:, 1:] = np.cumsum(txt != r[None, :], axis=1)
    p = np.arange(first, last + 1, dtype=np.int64)
    prow = p - q0
    rows = []
    for g in range(-gmax, gmax + 1):
        span = span_of(l, g)
        ok = p + span <= fe
        ok[ok] &= (t.ncum[p[ok] + span] - t.ncum[p[ok]]) == 0
        if not ok.any():
            continue
        jlo, jhi = split_range(l, g, prm)
        d = max(0, -g)
        js = np.arange(jlo, jhi + 1, dtype=np.int64)
        qrow = prow + g
        k = cum[prow][:, js] + cum[qrow, l][:, None] - cum[qrow][:, js + d] if g else cum[prow, l][:, None]
        cost = prm.cost_mismatch * k + (prm.cost_open + prm.cost_extend * abs(g) if g else 0)
        hit = ok[:, None] & (k <= 15) & (cost <= prm.max_cost)
        for a, b in zip(*np.nonzero(hit)):
            rows.append((int(cost[a, b]), abs(g), int(p[a]), g, int(js[b]), int(k[a, b])))
    return rows


def aligned_pairs(l, p, g, j):
    """the (read offset, text position) pairs of alignment (p, g, j) of a read of l bases"""
    if g == 0:
        return [(i, p + i) for i in range(l)]
    if g > 0:
        return [(i, p + i) for i in range(j)] + [(i, p + g + i) for i in range(j, l)]
    d = -g
    return [(i, p + i) for i in range(j)] + [(i, p + i - d) for i in range(j + d, l)]


def brute_candidates(t: Text, r, first, last, fs, fe, prm):
    l = int(r.shape[0])
    rows = []
    for p in range(first, last + 1):
        for g in range(-prm.max_gap, prm.max_gap + 1):
            span = span_of(l, g)
            if p < fs or p + span > fe or (t.sym[p:p + span] > 3).any():
                continue
            jlo, jhi = split_range(l, g, prm)
            for j in range(jlo, jhi + 1):
                al = aligned_pairs(l, p, g, j)
                assert al[-1][1] == p + span - 1 and len(al) == l - max(0, -g)
                k = sum(1 for i, x in al if r[i] != t.sym[x])
                c = cost_of(k, g, prm)
                if k <= 15 and c <= prm.max_cost:
                    rows.append((c, abs(g), p, g, j, k))
    return rows


def record_of(rows, prm, frag, fileid, target, inverted):
    """the record of a candidate set: sort the keys"""
    rec = empty_records(1)[0]
    if not rows:
        return rec
    rows = sorted(rows)
    cost, _, p, g, j, k = rows[0]
    others = [r[0] for r in rows if abs(r[2] - p) > prm.max_gap]
    second = min(others) if others else NONE
    state = NONUNIQUE if others and second <= cost + prm.margin else UNIQUE
    rec["pos"], rec["frag"], rec["fileid"], rec["split"], rec["gap"], rec["k"], rec["cost"], rec["second"] = p, frag, fileid, j, g, k, cost, second
    rec["tag"] = int(target) | (int(inverted) << 4) | (state << 5)
    return rec


def oriented(read, inverted):
    read = np.asarray(read, dtype=np.uint8)
    return COMP[read[::-1]] if inverted else read


def roles(pair_state, tag1, tag2):
    """(target mate, anchor mate) of a fragment, or None: the pair NoMatch, exactly one single Unique, the other NoMatch"""
    s1, s2 = int(state_of(tag1)), int(state_of(tag2))
    if int(pair_state) != NOMATCH or (s1 == UNIQUE) == (s2 == UNIQUE):
        return None
    tm = 1 if s1 == UNIQUE else 0
    return (tm, 1 - tm) if (s1, s2)[tm] == NOMATCH else None


def check_gap(t: Text, b1, b2, pairs, s1, s2, min_ins, max_ins, prm, out=None, candidates=cumsum_candidates):
    """(records, counters) of one call on the resident file t; out: the records to fold into (fresh = 0), None: fresh"""
    n = int(pairs.shape[0])
    fresh = out is None
    out = empty_records(n) if fresh else out.copy()
    ctr = dict.fromkeys(COUNTERS, 0)
    ctr["fragments"] = n
    mates, singles = (b1, b2), (s1, s2)
    for i in range(n):
        ro = roles(pairs["state"][i], s1["tag"][i], s2["tag"][i])
        if ro is None:
            continue
        tm, am = ro
        anchor = singles[am][i]
        if int(anchor["fileid"]) != t.fileid:
            ctr["other_file"] += 1
            continue
        ctr["eligible"] += 1
        out[i] = empty_records(1)[0]
        target = mates[tm].bases[int(mates[tm].offsets[i]):int(mates[tm].offsets[i + 1])]
        la = int(mates[am].offsets[i + 1]) - int(mates[am].offsets[i])
        l, a, frag, inv = int(target.shape[0]), int(anchor["pos"]), int(anchor["frag"]), int(inverted_of(anchor["tag"]))
        skip = l > MAX_PATL or l < 2 * prm.min_flank + prm.max_gap + 1 or (target > 3).any() or frag >= len(t.frag_start) - 1
        if not skip:
            fs, fe = t.frag_start[frag], t.frag_start[frag + 1]
            skip = a < fs or a + la > fe
        if skip:
            ctr["skipped"] += 1
            continue
        w = window(a, inv, la, l, min_ins, max_ins, prm.max_gap, fs, fe)
        if w is None:
            continue
        ctr["positions"] += w[1] - w[0] + 1
        rows = candidates(t, oriented(target, not inv), w[0], w[1], fs, fe, prm)
        out[i] = record_of(rows, prm, frag, t.fileid, tm, not inv)
        st = int(state_of(out[i]["tag"]))
        ctr["placed"] += st != NOMATCH
        ctr["unique"] += st == UNIQUE
        ctr["gapped"] += st != NOMATCH and int(out[i]["gap"]) != 0
    return out, ctr


def cigar_of(rec, l):
    g, j = int(rec["gap"]), int(rec["split"])
    if g == 0:
        return "%dM" % l
    return "%dM%dD%dM" % (j, g, l - j) if g > 0 else "%dM%dI%dM" % (j, -g, l - j + g)


def assert_records_equal(got, want, what=""):
    assert got.shape == want.shape, (got.shape, want.shape)
    for f in REC_DTYPE.names:
        bad = np.nonzero(np.asarray(got[f]) != np.asarray(want[f]))[0]
        assert bad.size == 0, "%s field %s differs at %d fragments, first %d: got %r want %r" % (what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])
