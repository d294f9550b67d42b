"""The checker of the paired-end tests -- TEST INFRASTRUCTURE ONLY.

A brute-force numpy statement of the semantics in include/real_hip.h ("paired-end reads") over hit lists in the form
oracle_lib.match_all returns them (or hand-made ones).  It never calls the code under test and imports nothing of the
product; the workloads the tests share are in pairs_workloads.py.
"""
from __future__ import annotations

import numpy as np

NOMATCH, UNIQUE, NONUNIQUE = 0, 1, 2
REC_DTYPE = np.dtype([("best", "<f8"), ("second", "<f8"), ("pos1", "<u4"), ("pos2", "<u4"), ("score1", "<f4"), ("score2", "<f4"),
                      ("frag", "<u2"), ("fileid", "u1"), ("k1", "u1"), ("k2", "u1"), ("inverted1", "u1"), ("state", "u1"),
                      ("reserved", "u1")])
FIELDS = [n for n in REC_DTYPE.names]
NINF = -np.inf


def eps_of(scores: bool, filter_mult: float, len1: int, len2: int) -> float:
    return float(np.float64(np.float32(np.float64(filter_mult) * np.float64(int(len1) + int(len2))))) if scores else 0.0


def concordant(h1, h2, l1, l2, min_ins, max_ins) -> bool:
    """h1 of mate 1, h2 of mate 2 (records with pos, frag, inverted)"""
    if int(h1["frag"]) != int(h2["frag"]) or bool(h1["inverted"]) == bool(h2["inverted"]):
        return False
    f, lf, r, lr = (h1, l1, h2, l2) if not h1["inverted"] else (h2, l2, h1, l1)
    fp, rp = int(f["pos"]), int(r["pos"])
    if fp > rp or fp + lf > rp + lr:
        return False
    return min_ins <= rp + lr - fp <= max_ins


def candidates(h1, h2, l1, l2, min_ins, max_ins, scores, fileid):
    """every concordant pair of the product as (value, location, payload)"""
    out = []
    for a in h1:
        for b in h2:
            if concordant(a, b, l1, l2, min_ins, max_ins):
                v = float(np.float64(a["score"]) + np.float64(b["score"])) if scores else -float(int(a["k"]) + int(b["k"]))
                loc = (int(fileid), int(a["frag"]), int(a["pos"]), int(b["pos"]), int(bool(a["inverted"])))
                out.append((v, loc, (np.float32(a["score"]), np.float32(b["score"]), int(a["k"]), int(b["k"]))))
    return out


def record_of(cands, eps):
    """top two of a set of candidates -> one record"""
    r = np.zeros((), dtype=REC_DTYPE)
    r["best"] = r["second"] = NINF
    if not cands:
        return r
    by_loc = {}
    for v, loc, pay in cands:                       # a set: a location counts once (its highest value)
        if loc not in by_loc or v > by_loc[loc][0]:
            by_loc[loc] = (v, pay)
    order = sorted(by_loc.items(), key=lambda kv: (-kv[1][0], kv[0]))
    loc, (v, pay) = order[0]
    second = order[1][1][0] if len(order) > 1 else NINF
    r["best"], r["second"] = v, second
    r["fileid"], r["frag"], r["pos1"], r["pos2"], r["inverted1"] = loc
    r["score1"], r["score2"], r["k1"], r["k2"] = pay
    r["state"] = NONUNIQUE if second >= v - eps else UNIQUE
    return r


def check_pairs(files, len1, len2, min_ins, max_ins, scores, filter_mult):
    """files: list of (fileid, hits1, off1, hits2, off2); the records of all fragments over the union of the files"""
    n = len(len1)
    out = np.zeros(n, dtype=REC_DTYPE)
    for i in range(n):
        cands = []
        for fid, h1, o1, h2, o2 in files:
            cands += candidates(h1[int(o1[i]):int(o1[i + 1])], h2[int(o2[i]):int(o2[i + 1])], int(len1[i]), int(len2[i]),
                                min_ins, max_ins, scores, fid)
        out[i] = record_of(cands, eps_of(scores, filter_mult, len1[i], len2[i]))
    return out


def naive_pairs(files, len1, len2, min_ins, max_ins, scores, filter_mult):
    """A second, deliberately different formulation: the two orientations are enumerated separately with the conditions
    written out on plain integers, the best and the runner-up are found by two linear scans."""
    n = len(len1)
    out = np.zeros(n, dtype=REC_DTYPE)
    for i in range(n):
        l1, l2 = int(len1[i]), int(len2[i])
        table = {}
        for fid, h1, o1, h2, o2 in files:
            A, B = h1[int(o1[i]):int(o1[i + 1])], h2[int(o2[i]):int(o2[i + 1])]
            for a in A:
                for b in B:
                    if a["frag"] != b["frag"]:
                        continue
                    ok = False
                    if a["inverted"] == 0 and b["inverted"] == 1:       # mate 1 forward
                        d = int(b["pos"]) + l2 - int(a["pos"])
                        ok = int(a["pos"]) <= int(b["pos"]) and int(a["pos"]) + l1 <= int(b["pos"]) + l2 and min_ins <= d <= max_ins
                    elif a["inverted"] == 1 and b["inverted"] == 0:     # mate 2 forward
                        d = int(a["pos"]) + l1 - int(b["pos"])
                        ok = int(b["pos"]) <= int(a["pos"]) and int(b["pos"]) + l2 <= int(a["pos"]) + l1 and min_ins <= d <= max_ins
                    if ok:
                        val = (np.float64(a["score"]) + np.float64(b["score"])) if scores else -np.float64(int(a["k"]) + int(b["k"]))   # (-0.0 for no mismatch at all, as -(double)(k1 + k2) is)
                        table[(fid, int(a["frag"]), int(a["pos"]), int(b["pos"]), int(a["inverted"]))] = (float(val), a, b)
        r = np.zeros((), dtype=REC_DTYPE)
        r["best"] = r["second"] = NINF
        best = None
        for loc, (v, a, b) in table.items():
            if best is None or v > table[best][0] or (v == table[best][0] and loc < best):
                best = loc
        if best is not None:
            v, a, b = table[best]
            second = NINF
            for loc, (w, _, _) in table.items():
                if loc != best and w > second:
                    second = w
            r["best"], r["second"] = v, second
            r["fileid"], r["frag"], r["pos1"], r["pos2"], r["inverted1"] = best
            r["score1"], r["score2"], r["k1"], r["k2"] = a["score"], b["score"], a["k"], b["k"]
            r["state"] = NONUNIQUE if second >= v - eps_of(scores, filter_mult, l1, l2) else UNIQUE
        out[i] = r
    return out


def loc_of(r):
    return (int(r["fileid"]), int(r["frag"]), int(r["pos1"]), int(r["pos2"]), int(r["inverted1"]))


def merge(a, b, eps):
    """top two of the union of two records' sets (the fold across genome files)"""
    a, b = a.copy(), b.copy()
    if b["best"] == NINF:
        out = a
    elif a["best"] == NINF:
        out = b
    elif loc_of(a) == loc_of(b):
        out = a if a["best"] >= b["best"] else b
        out["second"] = max(a["second"], b["second"])
    else:
        w, l = (a, b) if (-a["best"], loc_of(a)) < (-b["best"], loc_of(b)) else (b, a)
        out = w
        out["second"] = max(w["second"], l["best"])
    if out["best"] == NINF:
        out["state"] = NOMATCH
    else:
        out["state"] = NONUNIQUE if out["second"] >= out["best"] - eps else UNIQUE
    return out


def assert_records_equal(got, want, what=""):
    """every field, the FP64 values and the scores bit for bit"""
    assert got.shape == want.shape, (got.shape, want.shape)
    for f in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        if g.dtype.kind == "f":
            g, w = g.view("u%d" % g.dtype.itemsize), w.view("u%d" % w.dtype.itemsize)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s field %s differs at %d fragments, first %d: got %r want %r" % (
            what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])
