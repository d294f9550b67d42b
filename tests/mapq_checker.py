"""The checker of the mapping quality tests -- TEST INFRASTRUCTURE ONLY.

A brute-force statement of the semantics in include/real_hip.h ("mapping quality") in Python integers and math.floor, over
hit lists in the form oracle_lib.match_all returns them (or hand-made ones: any record array with pos, frag, inverted, k,
score).  It never calls the code under test and imports nothing of the product.  An accumulator is a dict {level, n, cnt}
(cnt a list of 32 ints); acc_records turns a list of them into the ABI's 40-byte records for bit-for-bit comparisons.
"""
from __future__ import annotations

import math

import numpy as np

LEVELS = 32
MISMATCH_LEVELS = 12
MAX_Q = 60
NONE = 255
EMPTY_LEVEL = -(1 << 31)
N_SAT = (1 << 32) - 1
ACC_DTYPE = np.dtype([("level", "<i4"), ("n", "<u4"), ("cnt", "u1", (LEVELS,))])


def _round_half_even_sqrt2_pow(j: int) -> int:
    """round(2^24 * 2^(-j/2)) in integers: exact for even j, through the integer square root for odd j"""
    if j % 2 == 0:
        return 1 << (24 - j // 2)
    # 2^24 * 2^(-j/2) = sqrt(2^(48 - j)); compare (2m + 1)^2 with 4 * 2^(48 - j) to round (never a tie: sqrt(2) is irrational)
    x = 1 << (48 - j)
    m = math.isqrt(x)
    return m + 1 if (2 * m + 1) ** 2 < 4 * x else m


W = [_round_half_even_sqrt2_pow(j) for j in range(LEVELS)]


def _a_of(q: int) -> int:
    """round(16 * 10^(q/10)) in integers: the integer m with (m - 1/2)^10 <= 16^10 * 10^q < (m + 1/2)^10"""
    target = (32 ** 10) * (10 ** q)           # (2 * 16)^10 * 10^q = (2 m')^10 for the real value m'
    lo, hi = 0, 1 << 40
    while lo < hi:                            # the largest m with (2m - 1)^10 <= target
        mid = (lo + hi + 1) // 2
        if (2 * mid - 1) ** 10 <= target:
            lo = mid
        else:
            hi = mid - 1
    return lo


A = [_a_of(q) for q in range(MAX_Q + 1)]


def level_of_value(v: float) -> int:
    f = math.floor(2.0 * float(v))
    return max(EMPTY_LEVEL + 1, min((1 << 31) - 1, f))


def level_of_k(k: int) -> int:
    return -MISMATCH_LEVELS * int(k)


def hit_level(h, scores) -> int:
    return level_of_value(float(np.float64(np.float32(h["score"])))) if scores else level_of_k(int(h["k"]))


def pair_level(a, b, scores) -> int:
    if scores:
        return level_of_value(float(np.float64(np.float32(a["score"])) + np.float64(np.float32(b["score"]))))
    return level_of_k(int(a["k"]) + int(b["k"]))


def empty():
    return {"level": EMPTY_LEVEL, "n": 0, "cnt": [0] * LEVELS}


def acc_of_levels(levels):
    """the accumulator of a multiset of levels, by its definition: the top, then a count per distance"""
    levels = [int(x) for x in levels]
    if not levels:
        return empty()
    top = max(levels)
    cnt = [0] * LEVELS
    for x in levels:
        if top - x < LEVELS:
            cnt[top - x] = min(255, cnt[top - x] + 1)
    return {"level": top, "n": min(N_SAT, len(levels)), "cnt": cnt}


def sorted_acc_of_levels(levels):
    """A second, deliberately different formulation: sort the levels descending, then count runs."""
    rows = sorted((int(x) for x in levels), reverse=True)
    a = empty()
    if not rows:
        return a
    a["level"], a["n"] = rows[0], min(N_SAT, len(rows))
    i = 0
    while i < len(rows) and rows[0] - rows[i] < LEVELS:
        j = i
        while j < len(rows) and rows[j] == rows[i]:
            j += 1
        a["cnt"][rows[0] - rows[i]] = min(255, j - i)
        i = j
    return a


def merge(a, b):
    """align to the larger level, shift the other down, add with saturation; an accumulator with n = 0 is empty"""
    a = a if a["n"] else empty()
    b = b if b["n"] else empty()
    top = max(a["level"], b["level"])
    cnt = [0] * LEVELS
    for x in (a, b):
        d = top - x["level"]
        for j, c in enumerate(x["cnt"]):
            if j + d < LEVELS:
                cnt[j + d] = min(255, cnt[j + d] + c)
    return {"level": top, "n": min(N_SAT, a["n"] + b["n"]), "cnt": cnt}


def quality(acc, lp: int):
    """(MAPQ, unlisted) of a placement of level lp"""
    acc = acc if acc["n"] else empty()
    j = acc["level"] - lp
    unlisted = j < 0 or j >= LEVELS or acc["cnt"][j] == 0
    if unlisted:
        acc = merge(acc, {"level": int(lp), "n": 1, "cnt": [1] + [0] * (LEVELS - 1)})
        j = acc["level"] - lp
    S = sum(c * w for c, w in zip(acc["cnt"], W))
    E = S - (W[j] if j < LEVELS else 0)
    return max(q for q in range(MAX_Q + 1) if E * A[q] <= 16 * S), unlisted


def acc_records(accs) -> np.ndarray:
    out = np.zeros(len(accs), dtype=ACC_DTYPE)
    for i, a in enumerate(accs):
        out[i]["level"], out[i]["n"], out[i]["cnt"] = a["level"], a["n"], a["cnt"]
    return out


def acc_from_record(r):
    return {"level": int(r["level"]), "n": int(r["n"]), "cnt": [int(c) for c in r["cnt"]]}


def concordant(a, b, la, lb, min_insert, max_insert) -> bool:
    """the paired-end block of include/real_hip.h: same frag, opposite strands, FR, outer distance within the bounds"""
    if int(a["frag"]) != int(b["frag"]) or bool(a["inverted"]) == bool(b["inverted"]):
        return False
    (f, lf), (r, lr) = ((a, la), (b, lb)) if not a["inverted"] else ((b, lb), (a, la))
    fp, rp = int(f["pos"]), int(r["pos"])
    if fp > rp or fp + int(lf) > rp + int(lr):
        return False
    return min_insert <= rp + int(lr) - fp <= max_insert


def hit_levels(hits, scores):
    if scores:
        return [level_of_value(x) for x in np.asarray(hits["score"], dtype=np.float32).astype(np.float64)]
    return [level_of_k(x) for x in hits["k"]]


def check_hits(blocks, n, scores, count=acc_of_levels):
    """blocks: list of (hits, off); the accumulators of n reads over the union of the blocks"""
    return [count([x for hits, off in blocks for x in hit_levels(hits[int(off[i]):int(off[i + 1])], scores)]) for i in range(n)]


def pair_levels(h1, h2, la, lb, min_insert, max_insert, scores):
    """the levels of the concordant pairs among (hits h1 of mate 1) x (hits h2 of mate 2): the whole product as one table.
    The same statement as concordant / pair_level, cell by cell (test_mapq_cpu.py holds the two against each other)."""
    if not len(h1) or not len(h2):
        return []
    a = {k: np.asarray(h1[k])[:, None] for k in ("frag", "inverted", "pos", "k")}
    b = {k: np.asarray(h2[k])[None, :] for k in ("frag", "inverted", "pos", "k")}
    a_fwd = a["inverted"] == 0
    ok = (a["frag"] == b["frag"]) & (a_fwd != (b["inverted"] == 0))
    fp = np.where(a_fwd, a["pos"], b["pos"]).astype(np.int64)
    rp = np.where(a_fwd, b["pos"], a["pos"]).astype(np.int64)
    lf, lr = np.where(a_fwd, int(la), int(lb)), np.where(a_fwd, int(lb), int(la))
    outer = rp + lr - fp
    ok &= (fp <= rp) & (fp + lf <= rp + lr) & (outer >= min_insert) & (outer <= max_insert)
    if scores:
        v = np.asarray(h1["score"], dtype=np.float32).astype(np.float64)[:, None] + np.asarray(h2["score"], dtype=np.float32).astype(np.float64)[None, :]
        return [level_of_value(x) for x in v[ok]]
    return [level_of_k(x) for x in (a["k"].astype(np.int64) + b["k"].astype(np.int64))[ok]]


def check_pair_hits(files, l1, l2, min_insert, max_insert, scores, count=acc_of_levels):
    """files: list of (h1, o1, h2, o2); the accumulators of the fragments over the concordant pairs inside each file"""
    out = []
    for i in range(len(l1)):
        levels = []
        for h1, o1, h2, o2 in files:
            levels += pair_levels(h1[int(o1[i]):int(o1[i + 1])], h2[int(o2[i]):int(o2[i + 1])], l1[i], l2[i], min_insert, max_insert, scores)
        out.append(count(levels))
    return out


def check_pair_hits_cellwise(files, l1, l2, min_insert, max_insert, scores, count=acc_of_levels):
    """the same, one cell of the product at a time (slow: for small lists)"""
    out = []
    for i in range(len(l1)):
        levels = []
        for h1, o1, h2, o2 in files:
            for a in h1[int(o1[i]):int(o1[i + 1])]:
                for b in h2[int(o2[i]):int(o2[i + 1])]:
                    if concordant(a, b, l1[i], l2[i], min_insert, max_insert):
                        levels.append(pair_level(a, b, scores))
        out.append(count(levels))
    return out


def finish_single(state, errors, score, accs, scores):
    """info records as (state, errors) arrays + scores -> (MAPQ bytes, placements, unlisted)"""
    out = np.full(len(accs), NONE, dtype=np.uint8)
    placed = unl = 0
    for i, a in enumerate(accs):
        if int(state[i]) in (1, 2):
            lp = level_of_value(float(np.float64(np.float32(score[i])))) if scores else level_of_k(int(errors[i]))
            out[i], u = quality(a, lp)
            placed, unl = placed + 1, unl + int(u)
    return out, placed, unl


def finish_pairs(pairs, s1, s2, acc_pair, acc1, acc2, scores):
    """pair records (best, k1, k2, state) and -- nullable -- the mates' singles (score, tag) -> (2n bytes, placements, unlisted)"""
    n = len(pairs)
    out = np.full(2 * n, NONE, dtype=np.uint8)
    placed = unl = 0
    for i in range(n):
        st = int(pairs["state"][i])
        if st == 1:
            lp = level_of_value(float(pairs["best"][i])) if scores else level_of_k(int(pairs["k1"][i]) + int(pairs["k2"][i]))
            q, u = quality(acc_pair[i], lp)
            out[2 * i] = out[2 * i + 1] = q
            placed, unl = placed + 2, unl + 2 * int(u)
        elif st == 0 and s1 is not None:
            for m, (s, acc) in enumerate(((s1, acc1), (s2, acc2))):
                tag = int(s["tag"][i])
                if (tag >> 5) & 3 == 1:
                    lp = level_of_value(float(np.float64(np.float32(s["score"][i])))) if scores else level_of_k(tag & 15)
                    out[2 * i + m], u = quality(acc[i], lp)
                    placed, unl = placed + 1, unl + int(u)
    return out, placed, unl
