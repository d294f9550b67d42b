"""Reads that steer real_hip_match_all's ordering pass (real_amd/csrc/all_order.hip) at its path edges -- TEST INFRASTRUCTURE
ONLY, pure numpy.  test_all_order_cpu.py shows with the oracle alone that the workload holds what it claims; test_gpu_all_order.py
compares the library with the oracle on it.

The pass has three paths by the hit count c of a read: 1 (straight to its place), 2 .. 32 (one lane per read), 33 .. 1024 (one
workgroup per read, quadratic rank) and beyond (workgroup radix sort by (k, pos), then the strand tie).  A read gets an exact
count from a tandem run of its own: a run of R bases of a unit of period p, flanked by 40 bases that differ from the run's
continuation at every base, holds floor((R - 38) / p) + 1 windows of 40 bases with at most two mismatches (p >= 3; the last
one overhangs the run by two bases: k = 2).  Two substitutions 15 bases apart mid-run leave the count as it is and give the
windows over them k = 1 and k = 2, so that the (k, pos) order of a read is not its position order.  A read of poly-A meets
EVERY poly-A run of a genome, so one genome gives that read one count: the run of 2101 bases (2066 hits, C flanks) is here as
the issue describes it, the other counts come from period-5 units that lie at least 8 mismatches from each other in every
rotation and on both strands.  Units that are their own reverse complement -- (AT), (CG) and the period-4 palindromes -- give
a forward and an inverted hit at every position: the tie (k, pos) leaves open.

`spread`: tandem repeats whose copies diverged by 4 % (reads of 100 bases, totalkmax 15) -- hundreds of hits per k, the
oracle's k-major order far from position order."""
from __future__ import annotations

import types

import numpy as np

from real_amd import synth

P, SEEDL, SEEDKMAX, K = 40, 16, 2, 2
SPREAD_P, SPREAD_K = 100, 15
FLANK, GAP = 40, 260
COUNTS = (0, 1, 2, 3, 31, 32, 33, 34, 255, 256, 257, 1023, 1024, 1025, 1026, 1279, 1280, 1281, 2066)
UNIT_COUNTS = (31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 255, 256, 257, 1023, 1024, 1025, 1026, 1279, 1280, 1281)   # period-5 runs
TIE_COUNTS = (32, 34, 256, 1024, 1026)                     # period-4 palindromes; (CG): 1280, (AT): 2066
POLY_R = 2101                                              # the poly-A and the (AT) run of the issue: 2066 hits each
SMALL_COPIES = (5, 10, 20, 30)
N_MULTI = 524_288 + 4096
N_BIG_SMALL, N_BIG_RADIX = 1024 + 76, 40
TOTALKMAX = {"edges": K, "edges_permuted": K, "many_big": K, "many_multi": K, "spread": SPREAD_K}


def _tile(unit, n, phase=0):
    p = len(unit)
    return np.asarray(unit, dtype=np.uint8)[(np.arange(n) + phase) % p]


def _min_dist(read, unit, skip_self=False, palindrome=False):
    """the fewest mismatches of `read` (or its reverse complement) against a run of `unit` in any rotation; skip_self leaves
    out the read's own alignment (rotation 0 forward; for a palindromic unit the inverted one as well)"""
    p = len(unit)
    t = _tile(unit, P + p)
    best = P
    for inv, r in ((0, read), (1, synth.revcomp(read))):
        for s in range(p):
            if skip_self and s == 0 and (inv == 0 or palindrome):
                continue
            best = min(best, int((t[s:s + P] != r).sum()))
    return best


def _pick_units(words, n, taken, palindrome=False):
    """the first n of `words` that lie 8 mismatches or more from every unit of `taken`, from each other and from their own
    rotations, on both strands"""
    out = []
    for w in words:
        if len(out) == n:
            break
        r = _tile(w, P)
        if _min_dist(r, w, True, palindrome) < 8:
            continue
        if all(_min_dist(r, u) >= 8 and _min_dist(_tile(u, P), w) >= 8 for u in taken + out):
            out.append(tuple(int(x) for x in w))
    assert len(out) == n, (len(out), n)
    return out


def _words(p, rng):
    w = np.array(np.unravel_index(np.arange(4 ** p), (4,) * p), dtype=np.uint8).T
    return w[rng.permutation(w.shape[0])]


def _run(rng, unit, R, flank_c=False, subs=True):
    """flank + run of R bases + flank -> (bases, offset of the run); a flank base is C or, drawn, any base but the one that
    would continue the run"""
    p = len(unit)
    seg = _tile(unit, R + 2 * FLANK, phase=(-FLANK) % p)
    out = seg.copy()
    for sl in (slice(0, FLANK), slice(FLANK + R, None)):
        out[sl] = 1 if flank_c else (seg[sl] + 1 + rng.integers(0, 3, size=FLANK)) & 3
    if subs and R >= 110:
        for j in (R // 2, R // 2 + 15):
            out[FLANK + j] = (out[FLANK + j] + 1) & 3
    return out, FLANK


def _diverged(rng, period, n, rate=0.04):
    unit = rng.integers(0, 4, size=period, dtype=np.uint8)
    seg = _tile(unit, n)
    return np.where(rng.random(n) < rate, rng.integers(0, 4, size=n, dtype=np.uint8), seg).astype(np.uint8)


def _qual(L):
    return (10 + np.arange(L) % 30).astype(np.uint8)


def _batch(reads):
    lens = [r.shape[0] for r in reads]
    return synth.ReadBatch(bases=np.concatenate(reads).astype(np.uint8), qual=np.concatenate([_qual(n) for n in lens]),
                           offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))


def read_of(b, i):
    return b.bases[int(b.offsets[i]):int(b.offsets[i + 1])]


_W = None


def workload():
    """-> namespace: g (two fragments); batch[name] = ReadBatch and meta[name][i] = (label, designed hit count or None, tie
    family, inverted) for "edges", "edges_permuted", "spread", "many_big"; kept = the reads of edges that edges_permuted
    holds, in its order; loci[label] = (start of the run, R, unit); many_multi() builds the largest batch on demand"""
    global _W
    if _W is not None:
        return _W
    rng = np.random.default_rng(4711)
    parts, loci, at = [], {}, [0]

    def put(seg):
        gap = rng.integers(0, 4, size=GAP, dtype=np.uint8)
        parts.extend([gap, seg])
        start = at[0] + GAP
        at[0] = start + seg.shape[0]
        return start

    def locus(label, unit, R, **kw):
        seg, o = _run(rng, unit, R, **kw)
        loci[label] = (put(seg) + o, R, tuple(unit))

    fixed = [(0,), (0, 3), (1, 2)]                                               # poly-A, (AT), (CG)
    pal4 = [w for w in _words(4, rng) if w[0] == 3 - w[3] and w[1] == 3 - w[2]]
    ties = _pick_units(pal4, len(TIE_COUNTS), fixed, palindrome=True)
    units = _pick_units(_words(5, rng), len(UNIT_COUNTS), fixed + ties)
    # first fragment: the period-5 runs
    for c, u in zip(UNIT_COUNTS, units):
        locus("u%d" % c, u, 38 + 5 * (c - 1))
    cut = put(np.zeros(0, np.uint8))
    # second fragment: the runs of the issue, the palindromes, the planted 40-mers, the diverged repeats
    locus("polyA", (0,), POLY_R, flank_c=True, subs=False)
    locus("AT", (0, 3), POLY_R, flank_c=True, subs=False)
    locus("CG", (1, 2), 34 + 1280, subs=False)
    for c, u in zip(TIE_COUNTS, ties):
        locus("t%d" % c, u, 34 + 2 * c, subs=False)
    x1, x2, x3 = (rng.integers(0, 4, size=P, dtype=np.uint8) for _ in range(3))
    for x, n in ((x1, 1), (x2, 2), (x3, 3)):
        for _ in range(n):
            put(x)
    d_rng = np.random.default_rng(5)
    spread_at = {"big": (put(_diverged(d_rng, 10, 15_000)), 15_000), "mid": (put(_diverged(d_rng, 10, 2000)), 2000)}
    for n in SMALL_COPIES:
        spread_at["small%d" % n] = (put(_diverged(d_rng, 10, SPREAD_P + 10 * n)), SPREAD_P + 10 * n)
    put(np.zeros(0, np.uint8))
    sym = np.concatenate(parts)
    g = synth.Genome(sym=sym, frag_start=np.array([0, cut, sym.shape[0]], dtype=np.uint64), frag_names=[" order_0", " order_1"])

    # ---- the distinct reads: (label, bases, designed count, tie, inverted) ----
    kinds = {}

    def kind(label, bases, count, tie=False):
        kinds[label] = (label, bases, count, tie, 0)
        if not tie:
            kinds[label + "-"] = (label + "-", synth.revcomp(bases), count, tie, 1)

    for c in UNIT_COUNTS:
        kind("u%d" % c, _tile(loci["u%d" % c][2], P), c)
    kind("polyA", _tile((0,), P), 2066)
    kind("AT", _tile((0, 3), P), 2066, tie=True)
    kind("CG", _tile((1, 2), P), 1280, tie=True)
    for c in TIE_COUNTS:
        kind("t%d" % c, _tile(loci["t%d" % c][2], P), c, tie=True)
    kind("x1", x1, 1)
    kind("x2", x2, 2)
    kind("x3", x3, 3)
    for i in range(4):
        kinds["none%d" % i] = ("none%d" % i, rng.integers(0, 4, size=P, dtype=np.uint8), 0, False, 0)

    def make(labels):
        return _batch([kinds[x][1] for x in labels]), [(kinds[x][0], kinds[x][2], kinds[x][3], kinds[x][4]) for x in labels]

    # ---- edges: every count; a radix read between a 1-hit and a 2-hit read; the last read is a radix read ----
    edge_counts = [c for c in UNIT_COUNTS if c not in (35, 36, 37, 38, 39, 40)]
    radix = [x for c in edge_counts if c > 1024 for x in ("u%d" % c, "u%d-" % c)] + ["polyA", "polyA-", "AT", "CG", "t1026"]
    rest = [x for c in edge_counts if c <= 1024 for x in ("u%d" % c, "u%d-" % c)] + ["t32", "t34", "t256", "t1024"]
    rest += ["x3", "x3-", "none0", "none1", "none2", "none3", "x1", "x2-"]
    rest = [rest[i] for i in rng.permutation(len(rest))]
    radix = [radix[i] for i in rng.permutation(len(radix))]
    labels = []
    for i, x in enumerate(radix[:-1]):
        labels += ["x1" if i % 2 == 0 else "x1-", x, "x2" if i % 4 < 2 else "x2-"] + rest[3 * i:3 * i + 3]
    labels += rest[3 * (len(radix) - 1):] + ["x1", radix[-1]]
    batch, meta = {}, {}
    batch["edges"], meta["edges"] = make(labels)
    kept = rng.permutation(len(labels))[:len(labels) - len(labels) // 4]
    batch["edges_permuted"], meta["edges_permuted"] = make([labels[i] for i in kept])

    # ---- many_big: 1100 reads of 33 .. 40 hits, 40 radix reads among them (half of them palindromes) ----
    big_radix = ["AT", "u1025", "t1026", "u1281-", "CG", "polyA-", "AT", "u1026-"]
    labels, step = [], N_BIG_SMALL // N_BIG_RADIX
    for i in range(N_BIG_SMALL):
        labels.append("u%d%s" % (33 + i % 8, "-" if (i // 8) % 2 else ""))
        if i % step == step - 1 and i // step < N_BIG_RADIX:
            labels.append(big_radix[(i // step) % len(big_radix)])
    batch["many_big"], meta["many_big"] = make(labels)

    # ---- spread: reads of 100 bases cut from the diverged repeats ----
    reads, smeta = [], []
    for name, offs in (("big", (1000, 7507, 12_006)), ("mid", (200, 903, 1606))):
        for o in offs:
            reads.append(sym[spread_at[name][0] + o:spread_at[name][0] + o + SPREAD_P].copy())
            smeta.append((name, None, False, 0))
    for n in SMALL_COPIES:
        s, ln = spread_at["small%d" % n]
        o = 10 * (n // 2)
        reads.append(sym[s + o:s + o + SPREAD_P].copy())
        smeta.append(("small", None, False, 0))
        reads.append(synth.revcomp(sym[s + o + 3:s + o + 3 + SPREAD_P]))
        smeta.append(("small", None, False, 1))
    order = [6, 0, 7, 3, 8, 1, 9, 4, 10, 2, 11, 5, 12, 13]
    batch["spread"], meta["spread"] = _batch([reads[i] for i in order]), [smeta[i] for i in order]
    _W = types.SimpleNamespace(g=g, loci=loci, batch=batch, meta=meta, kept=kept, kinds=kinds, cut=int(cut))
    return _W


# ---- many_multi: the lane grid's second trip ---------------------------------------------------------------------------
MULTI_KINDS = ("x2", "u33", "u1025")                        # 2 hits; every 1000th read 33 hits; every 50 000th 1025 hits
_M = None


def many_multi():
    """-> namespace: b (N_MULTI reads of 40 bases), distinct (the three reads it is made of, one each), kind[i] = which of the
    three read i is"""
    global _M
    if _M is None:
        w = workload()
        i = np.arange(N_MULTI)
        kind = np.zeros(N_MULTI, dtype=np.int64)
        kind[i % 1000 == 999] = 1
        kind[i % 50_000 == 2999] = 2
        three = np.stack([w.kinds[x][1] for x in MULTI_KINDS])
        bases = np.ascontiguousarray(three[kind]).reshape(-1)
        b = synth.ReadBatch(bases=bases, qual=np.tile(_qual(P), N_MULTI), offsets=(np.arange(N_MULTI + 1) * P).astype(np.uint64))
        _M = types.SimpleNamespace(b=b, distinct=_batch(list(three)), kind=kind)
    return _M


def head_of(b, n):
    """the first n reads of a batch"""
    e = int(b.offsets[n])
    return synth.ReadBatch(bases=b.bases[:e], qual=b.qual[:e], offsets=b.offsets[:n + 1])


def tiled(hits, hoff, kind):
    """the expected output of a batch whose read i is a copy of read kind[i] of the batch that (hits, hoff) answers: every
    read's list as it stands, the read index set -> (hits, offsets)"""
    hoff = hoff.astype(np.int64)
    cnt = np.diff(hoff)
    per = cnt[kind]
    off = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    out = np.zeros(int(off[-1]), dtype=hits.dtype)
    start = off[:-1].astype(np.int64)
    for k in range(cnt.shape[0]):
        idx = np.nonzero(kind == k)[0]
        if idx.size and cnt[k]:
            out[(start[idx][:, None] + np.arange(cnt[k])[None, :]).reshape(-1)] = np.tile(hits[hoff[k]:hoff[k + 1]], idx.size)
    out["read"] = np.repeat(np.arange(kind.shape[0], dtype=np.uint64), per)
    return out, off


# ---- the oracle on the workload, once per process ------------------------------------------------------------------------
_O = {}


def _ora_run(ora, b, totalkmax, scores):
    w = workload()
    if "g" not in _O:
        _O["g"] = ora.Genome(w.g.sym, w.g.frag_start)
        _O["ix"] = ora.Index(_O["g"], SEEDL)
    p = ora.make_params(seedl=SEEDL, seedkmax=SEEDKMAX, totalkmax=totalkmax, scores=scores)
    hits, hoff, ctr = ora.match_all(_O["g"], _O["ix"], p, b.bases, b.qual, b.offsets)
    return hits, hoff, ctr


def batch_of(name):
    return many_multi().b if name == "many_multi" else workload().batch[name]


def oracle(ora, name, scores=1):
    """-> namespace(hits, hoff, ctr) of ora.match_all on a batch; many_multi: the answer for its three distinct reads, tiled
    (ctr: the work of one copy of each read times the number of copies).  Nobody may change the arrays."""
    key = (name, scores)
    if key not in _O:
        if name == "many_multi":
            mm = many_multi()
            h3, o3, _ = _ora_run(ora, mm.distinct, K, scores)
            hits, hoff = tiled(h3, o3, mm.kind)
            n_of = np.bincount(mm.kind, minlength=3)
            ctr = {}
            for k in range(3):
                one = _ora_run(ora, head_of(synth.ReadBatch(bases=mm.distinct.bases[k * P:], qual=mm.distinct.qual[k * P:],
                                                            offsets=mm.distinct.offsets[:2]), 1), K, scores)[2]
                for f, v in one.items():
                    ctr[f] = ctr.get(f, 0) + int(v) * int(n_of[k])
        else:
            hits, hoff, ctr = _ora_run(ora, batch_of(name), TOTALKMAX[name], scores)
        for a in (hits, hoff):
            a.setflags(write=False)
        _O[key] = types.SimpleNamespace(hits=hits, hoff=hoff, ctr=ctr)
    return _O[key]
