"""Workloads the mate-search tests share (CPU test, GPU tests, CLI test) -- TEST INFRASTRUCTURE ONLY.

sample_pairs at a high substitution rate, plus planted fragments for every state change the search can cause.  A mate X
is hidden from the seeds by three substitutions inside its first seedl bases (the seed of both strands, in read
orientation); the other mate Y is found and anchors the search:
  A  NoMatch -> Unique      a fragment of unique text, X hidden
  B  NoMatch -> NonUnique   the same inside an exact two-copy family: X is placed beside both copies of Y
  C  Unique -> NonUnique    a stretch P copied to Q with six transitions inside X's footprint, three in its seed part and
                            three outside; X carries Q's bases outside the seed and P's inside: three mismatches at both,
                            found by the seeds at P only
  D  Unique -> Unique at a better location: as C, and Q differs from P in totalkmax more places inside Y's footprint,
                            which Y carries: the pair at Q has fewer mismatches, and only the search sees it
Every category cycles through X = mate 1 / mate 2 and X forward / reverse.
"""
from __future__ import annotations

import numpy as np

import mate_search_checker as mc

MIN_INS, MAX_INS, SEG_LEN, FRAG_L = 150, 420, 760, 300
PLANTS_PER_CATEGORY = 8
COMBOS = [(0, True), (1, True), (0, False), (1, False)]        # (X: index of the hidden mate, X is the forward mate)


def lens_of(b):
    return (b.offsets[1:] - b.offsets[:-1]).astype(np.uint32)


def search_workload(kind: str, ragged: bool, patl=(100, 80), seedl: int = 32, totalkmax: int = 3, n: int = 900, errprob: float = 0.04,
                    seed: int = 21, size: int = 300_000):
    """(genome, mate batch 1, mate batch 2, {category: [fragment indices planted]})"""
    from real_amd import synth
    families = (2, 2, 3) if kind == "iid" else (2, 3, 6, 30, 60)
    g, copies = synth.repeat_family_genome(size, seed, families=families, seg_len=SEG_LEN)
    kw = dict(insert_min=MIN_INS, insert_max=MAX_INS, copies=copies, seg_len=SEG_LEN, repeat_frac=0.1 if kind == "iid" else 0.3)
    p1 = synth.sample_pairs(g, n, patl[0], patl[1], 300, 30, errprob, seed + 3, **kw)
    if ragged:
        p2 = synth.sample_pairs(g, n // 2, 60, 120, 300, 30, errprob, seed + 4, **kw)
        b1, b2 = synth.ragged_pairs(p1, p2)
    else:
        b1, b2 = p1
    rng = np.random.default_rng(seed + 5)
    N = g.n
    busy = g.sym > 3
    for c in g.frag_start[1:-1]:
        busy[max(0, int(c) - 1):int(c) + 1] = True
    for fam in copies:
        for p in fam:
            busy[p:p + SEG_LEN] = True

    def free_spot(length):
        for _ in range(10_000):
            s = int(rng.integers(0, N - length))
            if not busy[s:s + length].any():
                busy[max(0, s - 2 * MAX_INS):s + length + 2 * MAX_INS] = True    # (far from every other plant)
                return s
        raise RuntimeError("no free spot")

    slots = [int(v) for v in np.linspace(3, b1.n_reads - 4, 4 * PLANTS_PER_CATEGORY).astype(int)]
    planted = {c: [] for c in "ABCD"}
    two = [fam for fam in copies if len(fam) == 2]
    lens = (lens_of(b1), lens_of(b2))
    for j, i in enumerate(slots):
        cat = "ABCD"[j % 4]
        X, xfwd = COMBOS[(j // 4) % 4]
        lx, ly = int(lens[X][i]), int(lens[1 - X][i])
        lf, lr = (lx, ly) if xfwd else (ly, lx)
        L = FRAG_L
        assert lf + lr <= L and lx >= seedl + 3 and ly >= seedl + totalkmax
        if cat == "B":
            fam = two[(j // 4) % len(two)]
            s = fam[0] + int(rng.integers(0, SEG_LEN - L))
        else:
            s = free_spot(L)
        xs, ys = (s, s + L - lr) if xfwd else (s + L - lr, s)                     # footprints of X and Y on the text
        seed_lo = xs if xfwd else xs + lx - seedl                                  # X's seed part on the text
        seed_at = seed_lo + rng.choice(seedl, size=3, replace=False)
        rest_lo = xs + seedl if xfwd else xs
        rest_at = rest_lo + rng.choice(lx - seedl, size=3, replace=False)
        y_rest_lo = ys if xfwd else ys + seedl                                     # Y's footprint without its seed part (Y is the other strand's mate)
        y_at = y_rest_lo + rng.choice(ly - seedl, size=totalkmax, replace=False)
        P = g.sym[s:s + L].copy()
        assert (P <= 3).all()
        xv, yv = P[xs - s:xs - s + lx].copy(), P[ys - s:ys - s + ly].copy()
        if cat in "AB":
            xv[seed_at - xs] ^= 2
        else:
            d = free_spot(L)
            Q = P.copy()
            Q[seed_at - s] ^= 2
            Q[rest_at - s] ^= 2
            xv[rest_at - xs] ^= 2
            if cat == "D":
                Q[y_at - s] ^= 2
                yv[y_at - ys] ^= 2
            g.sym[d:d + L] = Q
        x_read = xv if xfwd else mc.COMP[xv[::-1]]
        y_read = mc.COMP[yv[::-1]] if xfwd else yv
        for b, rd in ((b1, x_read if X == 0 else y_read), (b2, y_read if X == 0 else x_read)):
            lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
            assert hi - lo == len(rd)
            b.bases[lo:hi] = rd
            b.qual[lo:hi] = 35
        planted[cat].append(i)
    used = set(slots)
    for b, every in ((b1, 97), (b2, 131)):                          # reads the matcher skips: a symbol > 3
        for i in range(5, b.n_reads, every):
            if i not in used:
                b.bases[int(b.offsets[i]) + 7] = 4
    return g, b1, b2, planted


def oracle_lists(ora, g, b1, b2, seedl, totalkmax, scores, filter_level, fileid=0):
    """(fileid, hits1, off1, hits2, off2): the oracle's match_all lists of both mates for one genome file"""
    og = ora.Genome(g.sym, g.frag_start)
    ix = ora.Index(og, seedl)
    p = ora.make_params(seedl=seedl, seedkmax=2, totalkmax=totalkmax, scores=scores, filter_level=filter_level, fileid=fileid)
    h1, o1, _ = ora.match_all(og, ix, p, b1.bases, b1.qual, b1.offsets)
    h2, o2, _ = ora.match_all(og, ix, p, b2.bases, b2.qual, b2.offsets)
    return fileid, h1, o1, h2, o2


MIN_PER_TRANSITION = 5


def assert_coverage(off, on, f, what=""):
    """the conditions every parametrisation must meet, counted on the checker's records with and without the search
    (f: the oracle's lists the records were made from)"""
    tr = mc.transitions(off, on)
    counts = {k: int(v.size) for k, v in tr.items()}
    print(what, counts)
    for k, v in counts.items():
        assert v >= MIN_PER_TRANSITION, (what, k, counts)
    changed = np.concatenate(list(tr.values()))
    inv1 = on["inverted1"][changed]
    assert (inv1 == 0).any() and (inv1 == 1).any(), "both strands"
    _, h1, o1, h2, o2 = f
    searched = [0, 0]                                               # fragments whose reported placement of mate 1 / mate 2 is no seed hit
    for i in changed:
        r = on[i]
        for m, (h, o, pos, inv) in enumerate(((h1, o1, r["pos1"], r["inverted1"]), (h2, o2, r["pos2"], 1 - r["inverted1"]))):
            mine = h[int(o[i]):int(o[i + 1])]
            searched[m] += not ((mine["pos"] == pos) & (mine["inverted"] == inv)).any()
    assert searched[0] >= MIN_PER_TRANSITION and searched[1] >= MIN_PER_TRANSITION, ("either mate as the searched one", searched)
    return tr
