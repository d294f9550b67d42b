"""Hand-made anchors for real_hip_pair_search -- TEST INFRASTRUCTURE ONLY.

One fragment is one case: mate 1 and mate 2 are cut from the text at chosen positions (with chosen substitutions), one
or both of them are given as anchors (their true placements, scored by the checker's Searcher.placement), and the
search has to find -- or to refuse -- the other one.  The search needs the text only, no index, so such cases are cheap.
Expected records and counters come from mate_search_checker.search_only; the state written next to every case is what
its construction means, and is asserted against the checker before anything runs on a device.

Builder.add is the one way a case is made; the three case lists below use it:
  classic_cases   the insert bounds, the cut and the roles at 100 / 80 bases (test_gpu_mate_search.py)
  matrix_cases    every read width: the searched mate's length x the anchor's length x the placement's alignment x the
                  mismatch count, at forced substitution places
  geometry_cases  windows at the LDS bound, at the text's first and last base, at the cut, at the containment terms, at
                  the ends of partial 64-position chunks and next to an N; grouped by their insert bounds
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import mate_search_checker as mc
import pairs_checker as pc
from real_amd import synth

HIT = np.dtype([("pos", "<u4"), ("frag", "<u4"), ("inverted", "u1"), ("k", "u1"), ("score", "<f4")])
# a1 / a2: the anchors of mate 1 / mate 2 as (pos, frag, inverted, k, score); bounds: (min_insert, max_insert) of the call
Fragment = namedtuple("Fragment", "what r1 r2 a1 a2 state q1 q2 bounds")
U, NO = pc.UNIQUE, pc.NOMATCH
ANCHOR_COMBOS = [(0, False), (1, False), (0, True), (1, True)]     # (the anchor is mate 1 / mate 2, the anchor is the reverse mate)


def classic_genome():
    g = synth.random_genome(20_000, seed=77, n_frag=1)
    g.sym[g.sym > 3] = 0
    g.frag_start = np.array([0, 10_000, 20_000], dtype=np.uint64)
    g.frag_names = [" hand_0", " hand_1"]
    g.sym[3200] = 4                                                  # one N
    return g


N_AT = (3200, 8111, 23_456, 31_007)                                 # the single N's of wide_genome
WIDE_N, WIDE_CUT = 40_037, 19_983


def wide_genome():
    """two fragments, 40037 bases (neither a multiple of 32 nor of 64), the cut inside a word, four single N's"""
    assert WIDE_N % 32 and WIDE_N % 64 and WIDE_CUT % 32
    g = synth.random_genome(WIDE_N, seed=78, n_frag=1)
    g.sym[g.sym > 3] = 0
    g.frag_start = np.array([0, WIDE_CUT, WIDE_N], dtype=np.uint64)
    g.frag_names = [" wide_0", " wide_1"]
    g.sym[list(N_AT)] = 4
    return g


class Builder:
    """collects Fragments on one genome; qual: one quality for every base, or None: random per base, 0..63"""

    def __init__(self, g, S, seed, qual=30, l1=100, l2=80, bounds=None):
        self.g, self.S, self.qual, self.l1, self.l2, self.bounds = g, S, qual, l1, l2, bounds
        self.rng = np.random.default_rng(seed)
        self.qrng = np.random.default_rng(seed + 1000)
        self.F = []

    def text(self, p, ln):
        t = self.g.sym[p:p + ln].copy()
        t[t > 3] = 0
        return t

    def subs(self, rd, k, lo=0):
        rd = rd.copy()
        rd[lo + self.rng.choice(len(rd) - lo, size=k, replace=False)] ^= 2
        return rd

    def quals(self, ln):
        return np.full(ln, self.qual, np.uint8) if self.qual is not None else self.qrng.integers(0, 64, size=ln, dtype=np.uint8)

    def anchor(self, rd, q, inv, p):
        k, sc, frag = self.S.placement(rd, q, inv, p)
        return (p, frag, inv, k, float(sc))

    def add(self, what, p1, p2, fwd1, anchors, state, k1=0, k2=0, l1=None, l2=None, at1=None, at2=None, bounds=None):
        """mate 1 at p1 and mate 2 at p2 (text positions the reads are cut from), mate 1 forward or reverse; anchors: which
        mates are anchors; k1 / k2 random substitutions, or at1 / at2: substitutions at these offsets of the footprint"""
        l1, l2 = l1 or self.l1, l2 or self.l2
        r1, r2 = self.subs(self.text(p1, l1), k1), self.subs(self.text(p2, l2), k2)
        for r, at in ((r1, at1), (r2, at2)):
            if at is not None and len(at):
                assert len(set(at)) == len(at) and 0 <= min(at) and max(at) < len(r)
                r[list(at)] ^= 2
        r1, r2 = (r1, mc.COMP[r2[::-1]]) if fwd1 else (mc.COMP[r1[::-1]], r2)
        q1, q2 = self.quals(l1), self.quals(l2)
        a1 = [self.anchor(r1, q1, int(not fwd1), p1)] if 0 in anchors else []
        a2 = [self.anchor(r2, q2, int(fwd1), p2)] if 1 in anchors else []
        self.F.append(Fragment(what, r1, r2, a1, a2, state, q1, q2, bounds or self.bounds))

    def add_anchored(self, what, role, inva, pa, p, la, lb, state, at=None, bounds=None):
        """the anchor is mate role + 1, on the reverse strand if inva, at pa with la bases; the other mate (lb bases, cut
        from the text at p, substitutions at the offsets ``at`` of its footprint) is what the search looks for"""
        fwd1 = (role == 0) != bool(inva)
        p1, p2, l1, l2 = (pa, p, la, lb) if role == 0 else (p, pa, lb, la)
        self.add(what, p1, p2, fwd1, (role,), state, l1=l1, l2=l2, bounds=bounds, **{"at2" if role == 0 else "at1": at})


def batches(F):
    """(mate batch 1, mate batch 2, (hits 1, offsets 1), (hits 2, offsets 2)) of a list of Fragments"""
    def batch(rk, qk):
        rd = [f[rk] for f in F]
        off = np.cumsum([0] + [len(r) for r in rd]).astype(np.uint64)
        return synth.ReadBatch(bases=np.concatenate(rd).astype(np.uint8), qual=np.concatenate([f[qk] for f in F]).astype(np.uint8), offsets=off, ids=None)

    def lists(k):
        rows = [a for f in F for a in f[k]]
        h = np.zeros(len(rows), dtype=HIT)
        for j, (p, frag, inv, kk, sc) in enumerate(rows):
            h[j] = (p, frag, inv, kk, sc)
        return h, np.cumsum([0] + [len(f[k]) for f in F]).astype(np.uint64)
    return batch(1, 6), batch(2, 7), lists(3), lists(4)


def product_hits(h, dtype):
    """hits in the layout above -> records of ``dtype`` (the product's real_hip_hit)"""
    out = np.zeros(h.shape[0], dtype=dtype)
    for k in ("pos", "score", "frag", "k", "inverted"):
        out[k] = h[k]
    return out


def by_bounds(F):
    """{(min_insert, max_insert): [Fragments]} in first-seen order"""
    out = {}
    for f in F:
        out.setdefault(f.bounds, []).append(f)
    return out


# ---- the cases of test_gpu_mate_search.py ------------------------------------------------------------------------------
MIN_H, MAX_H, L1, L2 = 150, 420, 100, 80


def classic_cases(g, S, tk):
    B = Builder(g, S, 5, qual=30, l1=L1, l2=L2, bounds=(MIN_H, MAX_H))
    add = B.add
    # mate 1 forward at 1000 is the anchor; outer distance = p2 + L2 - 1000
    add("outer distance at the upper bound", 1000, 1000 + MAX_H - L2, True, (0,), U)
    add("one beyond the upper bound", 1000, 1001 + MAX_H - L2, True, (0,), NO)
    add("outer distance at the lower bound", 1000, 1000 + MIN_H - L2, True, (0,), U)
    add("one below the lower bound", 1000, 999 + MIN_H - L2, True, (0,), NO)
    add("the placement touches the fragment's last base", 9700, 10_000 - L2, True, (0,), U)
    add("an N inside the placement", 3000, 3150, True, (0,), NO)
    add("k == totalkmax", 5000, 5200, True, (0,), U, k2=tk)
    add("k == totalkmax + 1", 5000, 5200, True, (0,), NO, k2=tk + 1)
    # the anchor on either strand and of either mate
    add("anchor: mate 2, reverse", 6000, 6200, True, (1,), U, k1=2)
    add("anchor: mate 1, reverse", 7220, 7000, False, (0,), U, k2=1)
    add("anchor: mate 2, forward", 7220, 7000, False, (1,), U, k1=3)
    add("both mates anchor: one location", 8000, 8250, True, (0, 1), U)
    add("reverse anchor, outer distance at the upper bound", 12_000 + MAX_H - L1, 12_000, False, (0,), U)
    add("reverse anchor, one beyond", 12_001 + MAX_H - L1, 12_000, False, (0,), NO)
    add("reverse anchor at the fragment's first base", 10_200, 10_000, False, (0,), U)
    add("no anchors", 15_000, 15_200, True, (), NO)
    # one past the fragment's last base: mate 2 would straddle the cut at 10000 (its read is the text across it)
    add("one past the fragment's last base", 9700, 10_001 - L2, True, (0,), NO)
    return B.F


# ---- the length matrix -------------------------------------------------------------------------------------------------
LB_SET = (32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 191, 192, 193, 255, 256, 257, 288, 319, 320)
LA_SET = (32, 100, 320)
ALIGN_SET = (0, 1, 31)
MATRIX_TK = 3
MATRIX_BOUNDS = (32, 1100)
MatrixCell = namedtuple("MatrixCell", "la lb align k role inva p at")


def forced_subs(lb, k, j, rng):
    """k substitution places (offsets of the footprint, text order) from the read's first base, its last base and the two
    bases either side of a 32-base word boundary (the last boundary on odd j, any on even j).  k = totalkmax + 1 takes
    all four; k = totalkmax both ends and one side of the boundary, alternating.  A length without a boundary (32), or
    whose last base is one side of it (33, 65, ...: the other side is taken), is filled up from the other bases."""
    if k == 0:
        return []
    nw = (lb + 31) // 32
    want = [lb - 1, 0]
    if nw > 1:
        w = nw - 1 if j % 2 else 1 + (j // 2) % (nw - 1)
        sides = [32 * w - 1, 32 * w]
        side = sides[(j // 2) % 2]
        want += sides if k > MATRIX_TK else [side if side not in want else sides[1 - (j // 2) % 2]]
    at = []
    for x in want:
        if x not in at:
            at.append(x)
    while len(at) < k:
        x = int(rng.integers(1, lb - 1))
        if x not in at:
            at.append(x)
    return at[:k]


def matrix_cases(g, S, qual=None):
    """([Fragment], [MatrixCell]): 3 x 21 x 3 x 3 = 567 cases, the four anchor combinations cycled through them"""
    B = Builder(g, S, 6, qual=qual, bounds=MATRIX_BOUNDS)
    tk = MATRIX_TK
    fs = [int(v) for v in g.frag_start]
    cells, j = [], 0
    for la in LA_SET:
        for lb in LB_SET:
            for align in ALIGN_SET:
                for k in (0, tk, tk + 1):
                    role, inva = ANCHOR_COMBOS[j % 4]
                    f = (j // 4) % 2
                    d = max(la, lb) + int(B.rng.integers(0, 300))                  # the outer distance
                    while True:
                        p = int(B.rng.integers(fs[f] + 1200, fs[f + 1] - 1600))
                        p += align - p % 32
                        pa = p + d - la if inva else p + lb - d
                        if (g.sym[p:p + lb + 1] > 3).any() or (g.sym[pa:pa + la] > 3).any():
                            continue
                        if k == tk and g.sym[p + lb] == 0:                         # (a compare one base too far must count one more)
                            continue
                        break
                    at = forced_subs(lb, k, j, B.rng)
                    B.add_anchored("la %d lb %d align %d k %d anchor mate %d %s" % (la, lb, align, k, role + 1, "reverse" if inva else "forward"),
                                   role, inva, pa, p, la, lb, U if k <= tk else NO, at=at)
                    cells.append(MatrixCell(la, lb, align, k, role, inva, p, tuple(at)))
                    j += 1
    return B.F, cells


# ---- window geometry ---------------------------------------------------------------------------------------------------
def geometry_cases(g, S, lim, qual=None):
    """[Fragment], grouped by bounds; lim: the largest max_insert the search takes"""
    B = Builder(g, S, 7, qual=qual)
    n, cut = g.n, int(g.frag_start[1])
    sym = g.sym

    def clear(lo, hi):
        assert 0 <= lo and hi <= n and not (sym[lo:hi] > 3).any(), (lo, hi)

    def aligned(x, r):
        return x + (r - x) % 32
    # a full-width window at the limit, 320 + 320: lo mod 32 = 0, 1, 31; the mate at lo and at hi
    bw = (200, lim)
    for r in (0, 1, 31):
        for where in ("lo", "hi"):
            pa = aligned(2000, r)                                                  # forward anchor: lo = pa, hi = pa + lim - 320
            p = pa if where == "lo" else pa + lim - 320
            assert mc.window_of(pa, 320, 320, 0, 0, cut, *bw) == (pa, pa + lim - 320)
            B.add_anchored("full window, forward anchor, lo mod 32 = %d, mate at %s" % (r, where), 0, False, pa, p, 320, 320, U, at=[319] if where == "hi" else [0], bounds=bw)
            pa = aligned(cut + 9000, r)                                            # reverse anchor: hi = pa, lo = pa + 320 - lim
            p = pa if where == "hi" else pa + 320 - lim
            assert mc.window_of(pa, 320, 320, 1, cut, n, *bw) == (pa + 320 - lim, pa) and (pa + 320 - lim) % 32 == r
            B.add_anchored("full window, reverse anchor, lo mod 32 = %d, mate at %s" % (r, where), 1, True, pa, p, 320, 320, U, at=[319] if where == "hi" else [0], bounds=bw)
    # the most positions: 32 + 32 at the limit (lim - 31 of them)
    bs = (32, lim)
    for r in (31, 0):
        pa = aligned(9000, r)
        assert mc.window_of(pa, 32, 32, 0, 0, cut, *bs) == (pa, pa + lim - 32)
        B.add_anchored("32 + 32 at the limit, forward anchor, lo mod 32 = %d, mate at hi" % r, 1, False, pa, pa + lim - 32, 32, 32, U, at=[31], bounds=bs)
        pa = aligned(cut + 6000, r)
        assert mc.window_of(pa, 32, 32, 1, cut, n, *bs) == (pa + 32 - lim, pa)
        B.add_anchored("32 + 32 at the limit, reverse anchor, lo mod 32 = %d, mate at lo" % r, 0, True, pa, pa + 32 - lim, 32, 32, U, at=[0], bounds=bs)
    # window lengths 0, 1 and 63 mod 64, the placement at hi: the last lane of a whole chunk, a chunk of one, lane 62
    for span in (64, 65, 127, 128 + 63):
        b = (200, 200 + span - 1)
        pa = 4000 + span
        lo, hi = mc.window_of(pa, 100, 129, 0, 0, cut, *b)
        assert hi - lo + 1 == span
        B.add_anchored("window of %d positions, forward anchor, mate at hi" % span, span % 2, False, pa, hi, 100, 129, U, at=[128, 64], bounds=b)
        pa = cut + 5000 + span
        lo, hi = mc.window_of(pa, 100, 129, 1, cut, n, *b)
        assert hi - lo + 1 == span
        B.add_anchored("window of %d positions, reverse anchor, mate at hi" % span, 1 - span % 2, True, pa, hi, 100, 129, U, at=[0, 63], bounds=b)
    # the rest under the matrix's bounds
    B.bounds = MATRIX_BOUNDS
    mn, mx = MATRIX_BOUNDS
    # the text's first and last base, the cut from both sides and one past it on both sides
    for la, lb in ((100, 65), (65, 160)):
        t = "%d + %d" % (la, lb)
        assert mc.window_of(500, la, lb, 1, 0, cut, mn, mx)[0] == 0 > 500 + la - mx
        B.add_anchored(t + ": reverse anchor, window clipped by the text's first base, mate at 0", 0, True, 500, 0, la, lb, U, at=[0, lb - 1])
        pa = n - 700
        assert mc.window_of(pa, la, lb, 0, cut, n, mn, mx)[1] == n - lb < pa + mx - lb
        B.add_anchored(t + ": forward anchor, window clipped by the text's last base, mate ends there", 1, False, pa, n - lb, la, lb, U, at=[0, lb - 1])
        B.add_anchored(t + ": forward anchor, mate ends at the cut", 0, False, cut - 600, cut - lb, la, lb, U, at=[lb - 1])
        B.add_anchored(t + ": forward anchor, mate one past the cut", 1, False, cut - 600, cut - lb + 1, la, lb, NO)
        B.add_anchored(t + ": reverse anchor, mate starts at the cut", 1, True, cut + 600, cut, la, lb, U, at=[0])
        B.add_anchored(t + ": reverse anchor, mate one in front of the cut", 0, True, cut + 600, cut - 1, la, lb, NO)
    # containment: a forward anchor asks pa <= p and pa + la <= p + lb, a reverse one p <= pa and p + lb <= pa + la; which
    # of the two binds depends on lb > la or lb < la -- all four, with the position one outside each
    for la, lb in ((64, 193), (193, 64)):
        t = "%d + %d" % (la, lb)
        pa = 12_001
        lo = mc.window_of(pa, la, lb, 0, 0, cut, mn, mx)[0]
        assert lo == max(pa, pa + la - lb) and pa + mn - lb < lo
        clear(lo - 1, lo + lb)
        B.add_anchored(t + ": forward anchor, mate at the containment bound", 0, False, pa, lo, la, lb, U, at=[0])
        B.add_anchored(t + ": forward anchor, mate one outside the containment bound", 1, False, pa, lo - 1, la, lb, NO)
        pa = cut + 12_031
        hi = mc.window_of(pa, la, lb, 1, cut, n, mn, mx)[1]
        assert hi == min(pa, pa + la - lb) and pa + la - mn > hi
        clear(hi, hi + lb + 1)
        B.add_anchored(t + ": reverse anchor, mate at the containment bound", 1, True, pa, hi, la, lb, U, at=[lb - 1])
        B.add_anchored(t + ": reverse anchor, mate one outside the containment bound", 0, True, pa, hi + 1, la, lb, NO)
    # an N in the placement's first or last base is refused, an N one base outside either end is not
    for z, lb, inva in ((N_AT[1], 97, False), (N_AT[2], 128, True)):
        assert sym[z] == 4
        for what, p, state in (("N in the last base", z - lb + 1, NO), ("N in the first base", z, NO),
                               ("N one in front of the first base", z + 1, U), ("N one behind the last base", z - lb, U)):
            pa = p - 300 if not inva else p + 300
            clear(pa, pa + 100)
            B.add_anchored("%s, lb %d, %s anchor" % (what, lb, "reverse" if inva else "forward"), int(inva), inva, pa, p, 100, lb, state)
    return B.F
