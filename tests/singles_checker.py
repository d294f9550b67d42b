"""The checker of the tests of the single placements of a mate -- TEST INFRASTRUCTURE ONLY.

A brute-force numpy statement of the semantics in include/real_hip.h ("single placements of a mate") over hit lists in the
form oracle_lib.match_all returns them (or hand-made ones: any record array with pos, frag, inverted, k, score).  It never
calls the code under test and imports nothing of the product.
"""
from __future__ import annotations

import numpy as np

NOMATCH, UNIQUE, NONUNIQUE = 0, 1, 2
REC_DTYPE = np.dtype([("score", "<f4"), ("second", "<f4"), ("pos", "<u4"), ("frag", "<u2"), ("fileid", "u1"), ("tag", "u1")])
FIELDS = list(REC_DTYPE.names)
NINF = -np.inf


def k_of(tag):
    return np.asarray(tag) & 15


def inverted_of(tag):
    return (np.asarray(tag) >> 4) & 1


def state_of(tag):
    return (np.asarray(tag) >> 5) & 3


def make_tag(k, inverted, state):
    return (int(k) & 15) | (int(bool(inverted)) << 4) | (int(state) << 5)


def eps_of(scores: bool, filter_mult: float, length: int) -> float:
    return float(np.float64(np.float32(np.float64(filter_mult) * np.float64(int(length))))) if scores else 0.0


def value_of(h, scores) -> float:
    """(double)score, or -(double)k: -0.0 for k = 0"""
    return float(np.float64(np.float32(h["score"]))) if scores else float(-np.float64(int(h["k"])))


def _neg_zero_first(v: float):
    """among equal values the record's `second` prefers -0.0 to +0.0 (the only equal values with different bits)"""
    return 0 if np.signbit(v) else 1


def candidates(hits, scores, fileid):
    """every hit as (value, location, payload)"""
    return [(value_of(h, scores), (int(fileid), int(h["frag"]), int(h["pos"]), int(bool(h["inverted"]))), (np.float32(h["score"]), int(h["k"])))
            for h in hits]


def empty_record():
    r = np.zeros((), dtype=REC_DTYPE)
    r["second"] = NINF
    return r


def record_of(cands, eps):
    """top two of a set of candidates -> one record"""
    r = empty_record()
    if not cands:
        return r
    by_loc = {}
    for v, loc, pay in cands:                       # a set: a location counts once
        if loc not in by_loc or v > by_loc[loc][0]:
            by_loc[loc] = (v, pay)
    best = None
    for loc, (v, _) in by_loc.items():
        if best is None or v > by_loc[best][0] or (v == by_loc[best][0] and loc < best):
            best = loc
    v, (score, k) = by_loc[best]
    second = NINF
    for loc, (w, _) in by_loc.items():
        if loc != best and (w > second or (w == second and _neg_zero_first(w) < _neg_zero_first(second))):
            second = w
    state = NONUNIQUE if np.float64(second) >= np.float64(v) - np.float64(eps) else UNIQUE
    r["score"], r["second"] = score, np.float32(second)
    r["fileid"], r["frag"], r["pos"] = best[0], best[1], best[2]
    r["tag"] = make_tag(k, best[3], state)
    return r


def check_singles(files, lens, scores, filter_mult):
    """files: list of (fileid, hits, off); the records of all reads over the union of the files"""
    n = len(lens)
    out = np.zeros(n, dtype=REC_DTYPE)
    for i in range(n):
        cands = []
        for fid, h, o in files:
            cands += candidates(h[int(o[i]):int(o[i + 1])], scores, fid)
        out[i] = record_of(cands, eps_of(scores, filter_mult, lens[i]))
    return out


def sorted_singles(files, lens, scores, filter_mult):
    """A second, deliberately different formulation: all hits of a read as rows of (-value, sign, location), sorted; the
    first row is the best, the first later row at another location gives `second`."""
    n = len(lens)
    out = np.zeros(n, dtype=REC_DTYPE)
    for i in range(n):
        rows = []
        for fid, h, o in files:
            for x in h[int(o[i]):int(o[i + 1])]:
                val = np.float64(np.float32(x["score"])) if scores else -np.float64(int(x["k"]))
                rows.append((-float(val), 0 if np.signbit(val) else 1, int(fid), int(x["frag"]), int(x["pos"]), int(x["inverted"] != 0),
                             float(val), np.float32(x["score"]), int(x["k"])))
        # (the sign column orders -0.0 in front of +0.0 among equal values; the best is chosen by value and location alone)
        r = empty_record()
        if rows:
            rows.sort(key=lambda t: (t[0], t[2:6]))
            b = rows[0]
            others = sorted((t for t in rows if t[2:6] != b[2:6]), key=lambda t: (t[0], t[1]))
            second = others[0][6] if others else NINF
            eps = eps_of(scores, filter_mult, lens[i])
            r["score"], r["second"], r["fileid"], r["frag"], r["pos"] = b[7], np.float32(second), b[2], b[3], b[4]
            r["tag"] = make_tag(b[8], b[5], NONUNIQUE if second >= b[6] - eps else UNIQUE)
        out[i] = r
    return out


def loc_of(r):
    return (int(r["fileid"]), int(r["frag"]), int(r["pos"]), int(inverted_of(r["tag"])))


def _value_of_record(r, scores) -> float:
    return float(np.float64(r["score"])) if scores else float(-np.float64(int(k_of(r["tag"]))))


def _max2(a: float, b: float) -> float:
    if a > b:
        return a
    if b > a:
        return b
    return a if _neg_zero_first(a) <= _neg_zero_first(b) else b


def merge(a, b, scores, eps):
    """top two of the union of two records' sets (the fold across genome files and index blocks)"""
    a, b = a.copy(), b.copy()
    ea, eb = state_of(a["tag"]) == NOMATCH, state_of(b["tag"]) == NOMATCH
    if ea and eb:
        return empty_record()
    if eb:
        out, second = a, float(a["second"])
    elif ea:
        out, second = b, float(b["second"])
    elif loc_of(a) == loc_of(b):
        out, second = a, _max2(float(a["second"]), float(b["second"]))
    else:
        va, vb = _value_of_record(a, scores), _value_of_record(b, scores)
        w, lv = (a, vb) if (-va, loc_of(a)) < (-vb, loc_of(b)) else (b, va)
        out, second = w, _max2(float(w["second"]), lv)
    best = _value_of_record(out, scores)
    out["second"] = np.float32(second)
    out["tag"] = make_tag(k_of(out["tag"]), inverted_of(out["tag"]), NONUNIQUE if second >= best - eps else UNIQUE)
    return out


def assert_singles_equal(got, want, what=""):
    """every field, the floats bit for bit"""
    assert got.shape == want.shape, (got.shape, want.shape)
    for f in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        if g.dtype.kind == "f":
            g, w = g.view("u%d" % g.dtype.itemsize), w.view("u%d" % w.dtype.itemsize)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s field %s differs at %d reads, first %d: got %r want %r" % (
            what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])


def classes(pair_state, s1, s2):
    """what a parametrisation must contain among the fragments whose pair record is NoMatch, from the checker's records"""
    nm = np.asarray(pair_state) == NOMATCH
    u1, u2 = state_of(s1["tag"]) == UNIQUE, state_of(s2["tag"]) == UNIQUE
    n1, n2 = state_of(s1["tag"]) == NONUNIQUE, state_of(s2["tag"]) == NONUNIQUE
    e1, e2 = state_of(s1["tag"]) == NOMATCH, state_of(s2["tag"]) == NOMATCH
    return {"both_unique": int((nm & u1 & u2).sum()), "one_unique": int((nm & (u1 != u2)).sum()),
            "a_nonunique": int((nm & (n1 | n2)).sum()), "neither": int((nm & e1 & e2).sum())}
