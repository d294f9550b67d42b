"""The checker of the tests of the paired-end enumeration (every concordant pair of a fragment) -- TEST INFRASTRUCTURE ONLY.

A brute-force statement of include/real_hip.h ("every concordant pair of a fragment") over hit lists in the form
oracle_lib.match_all returns them (or hand-made ones): the product of a fragment's two lists is walked row-major and
every cell that pairs_checker.concordant accepts becomes one record.  It never calls the code under test and imports
nothing of the product.
"""
from __future__ import annotations

import numpy as np

from pairs_checker import NINF, concordant

LANE_BUDGET = 32        # a product beyond it is handed to a wave (the statistics count such fragments)
PAIR_HIT_DTYPE = np.dtype([("pair", "<u4"), ("pos1", "<u4"), ("pos2", "<u4"), ("outer", "<u4"), ("score1", "<f4"), ("score2", "<f4"),
                           ("frag", "<u2"), ("fileid", "u1"), ("inverted1", "u1"), ("k1", "u1"), ("k2", "u1"), ("reserved", "<u2")])
FIELDS = list(PAIR_HIT_DTYPE.names)
_HIT = ("pos", "score", "frag", "k", "inverted")


def _rows(h):
    """hit records as plain dicts (concordant() only indexes them); the scores stay float32 bit patterns"""
    cols = {f: h[f].tolist() for f in ("pos", "frag", "k", "inverted")}
    bits = np.ascontiguousarray(h["score"]).view(np.uint32).tolist()
    return [{"pos": cols["pos"][j], "frag": cols["frag"][j], "k": cols["k"][j], "inverted": cols["inverted"][j], "bits": bits[j]}
            for j in range(len(bits))]


def enumerate_pairs(h1, o1, len1, h2, o2, len2, min_ins, max_ins, fileid=0):
    """-> (records, offsets): every concordant pair of every fragment; inside a fragment ascending index of the mate-1
    hit, then ascending index of the mate-2 hit"""
    n = len(len1)
    R1, R2 = _rows(h1), _rows(h2)
    rows, off = [], np.zeros(n + 1, dtype=np.uint64)
    for i in range(n):
        l1, l2 = int(len1[i]), int(len2[i])
        B = R2[int(o2[i]):int(o2[i + 1])]
        for a in R1[int(o1[i]):int(o1[i + 1])]:
            for b in B:
                if concordant(a, b, l1, l2, min_ins, max_ins):
                    f, lf, r, lr = (a, l1, b, l2) if not a["inverted"] else (b, l2, a, l1)
                    rows.append((i, a["pos"], b["pos"], r["pos"] + lr - f["pos"], a["bits"], b["bits"], a["frag"], fileid,
                                 1 if a["inverted"] else 0, a["k"], b["k"], 0))
        off[i + 1] = len(rows)
    out = np.zeros(len(rows), dtype=PAIR_HIT_DTYPE)
    if rows:
        cols = list(zip(*rows))
        for f, c in zip(FIELDS, cols):
            if f in ("score1", "score2"):
                out[f] = np.array(c, dtype=np.uint32).view(np.float32)
            else:
                out[f] = np.array(c, dtype=np.uint64).astype(PAIR_HIT_DTYPE[f])
    return out, off


def enumerate_pairs_flat(h1, o1, len1, h2, o2, len2, min_ins, max_ins, fileid=0):
    """A second, deliberately different formulation: per fragment the FLATTENED cell index c = x * n2 + y is walked with
    numpy, the two orientations are tested separately on plain integer arrays, and the surviving cells are taken in
    ascending c."""
    n = len(len1)
    parts, off = [], np.zeros(n + 1, dtype=np.uint64)
    total = 0
    for i in range(n):
        A, B = h1[int(o1[i]):int(o1[i + 1])], h2[int(o2[i]):int(o2[i + 1])]
        n1, n2 = len(A), len(B)
        if n1 and n2:
            c = np.arange(n1 * n2, dtype=np.int64)
            a, b = A[c // n2], B[c % n2]
            l1, l2 = int(len1[i]), int(len2[i])
            p1, p2 = a["pos"].astype(np.int64), b["pos"].astype(np.int64)
            d_fwd1 = p2 + l2 - p1              # mate 1 forward
            d_fwd2 = p1 + l1 - p2              # mate 2 forward
            ok1 = (a["inverted"] == 0) & (b["inverted"] == 1) & (p1 <= p2) & (p1 + l1 <= p2 + l2) & (d_fwd1 >= min_ins) & (d_fwd1 <= max_ins)
            ok2 = (a["inverted"] == 1) & (b["inverted"] == 0) & (p2 <= p1) & (p2 + l2 <= p1 + l1) & (d_fwd2 >= min_ins) & (d_fwd2 <= max_ins)
            keep = (a["frag"] == b["frag"]) & (ok1 | ok2)
            a, b = a[keep], b[keep]
            r = np.zeros(int(keep.sum()), dtype=PAIR_HIT_DTYPE)
            r["pair"], r["pos1"], r["pos2"] = i, a["pos"], b["pos"]
            r["outer"] = np.where(ok1[keep], d_fwd1[keep], d_fwd2[keep])
            r["score1"], r["score2"], r["frag"], r["fileid"] = a["score"], b["score"], a["frag"], fileid
            r["inverted1"], r["k1"], r["k2"] = a["inverted"] != 0, a["k"], b["k"]
            parts.append(r)
            total += r.shape[0]
        off[i + 1] = total
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=PAIR_HIT_DTYPE)), off


def products(o1, o2):
    """the product of every fragment's list sizes"""
    return (np.asarray(o1[1:], dtype=np.int64) - np.asarray(o1[:-1], dtype=np.int64)) * \
           (np.asarray(o2[1:], dtype=np.int64) - np.asarray(o2[:-1], dtype=np.int64))


def expected_stats(o1, o2, recs):
    p = products(o1, o2)
    return {"products": int(p.sum()), "pairs_out": int(recs.shape[0]), "handed_over": int((p > LANE_BUDGET).sum())}


def value_of(r, scores):
    return float(np.float64(r["score1"]) + np.float64(r["score2"])) if scores else -float(int(r["k1"]) + int(r["k2"]))


def loc_of(r):
    return (int(r["fileid"]), int(r["frag"]), int(r["pos1"]), int(r["pos2"]), int(r["inverted1"]))


def top_two(recs, scores):
    """a fragment's enumerated pairs reduced under (value descending, location ascending):
    (best value, best record, second value) or (-inf, None, -inf)"""
    if recs.shape[0] == 0:
        return NINF, None, NINF
    order = sorted(range(recs.shape[0]), key=lambda j: (-value_of(recs[j], scores), loc_of(recs[j])))
    second = value_of(recs[order[1]], scores) if len(order) > 1 else NINF
    return value_of(recs[order[0]], scores), recs[order[0]], second


def assert_consistent_with_records(recs, off, records, scores, what=""):
    """the per-fragment records of the join (pairs_checker.REC_DTYPE layout) follow from the enumerated list: best value,
    its location and payload, and the second value"""
    for i in range(records.shape[0]):
        best, r, second = top_two(recs[int(off[i]):int(off[i + 1])], scores)
        R = records[i]
        assert np.float64(R["best"]) == np.float64(best) or (r is None and np.isneginf(R["best"])), (what, i, R, best)
        assert (np.isneginf(R["second"]) and second == NINF) or np.float64(R["second"]) == np.float64(second), (what, i, R, second)
        if r is not None:
            assert (int(R["fileid"]), int(R["frag"]), int(R["pos1"]), int(R["pos2"]), int(R["inverted1"])) == loc_of(r), (what, i, R, r)
            assert (int(R["k1"]), int(R["k2"])) == (int(r["k1"]), int(r["k2"])), (what, i)
            assert np.float32(R["score1"]).view(np.uint32) == np.float32(r["score1"]).view(np.uint32), (what, i)
            assert np.float32(R["score2"]).view(np.uint32) == np.float32(r["score2"]).view(np.uint32), (what, i)


def assert_pair_hits_equal(got, want, what=""):
    """every field, the scores bit for bit"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        if g.dtype.kind == "f":
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s field %s differs at %d pairs, first %d: got %r want %r" % (what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])
