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

The geometry is an argument: the insert bounds, the planted fragment length, the insert mean / sd of the sampled pairs
and the length pair(s) of the ragged second part.  The defaults are the module constants, and give the inputs every
earlier caller has always had (test_workload_defaults_cpu.py holds their hashes).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import mate_search_checker as mc

MIN_INS, MAX_INS, SEG_LEN, FRAG_L = 150, 420, 760, 300
PLANTS_PER_CATEGORY = 8
COMBOS = [(0, True), (1, True), (0, False), (1, False)]        # (X: index of the hidden mate, X is the forward mate)


def lens_of(b):
    return (b.offsets[1:] - b.offsets[:-1]).astype(np.uint32)


def ragged_parts(synth, g, n, ragged_patl, insert_mean, insert_sd, errprob, seed, kw):
    """the ragged second part of a workload: n fragments of one length pair, or of several in equal shares (the sampled
    inserts are no shorter than the longer mate)"""
    if isinstance(ragged_patl[0], int):
        return synth.sample_pairs(g, n, ragged_patl[0], ragged_patl[1], insert_mean, insert_sd, errprob, seed, **kw)
    parts = []
    for j, (l1, l2) in enumerate(ragged_patl):
        kj = dict(kw, insert_min=max(kw["insert_min"], l1, l2))
        parts.append(synth.sample_pairs(g, max(1, n // len(ragged_patl)), l1, l2, max(insert_mean, l1, l2), insert_sd, errprob, seed + 100 * j, **kj))
    return synth.concat_batches([p[0] for p in parts]), synth.concat_batches([p[1] for p in parts])


def random_qualities(batches, keep, seed):
    """per-base qualities uniform in 0..63 for every read but those of the fragments in ``keep``"""
    rng = np.random.default_rng(seed)
    for b in batches:
        q = rng.integers(0, 64, size=b.qual.shape[0], dtype=np.uint8)
        for i in keep:
            q[int(b.offsets[i]):int(b.offsets[i + 1])] = b.qual[int(b.offsets[i]):int(b.offsets[i + 1])]
        b.qual[:] = q


def search_workload(kind: str, ragged: bool, patl=(100, 80), seedl: int = 32, totalkmax: int = 3, n: int = 900, errprob: float = 0.04,
                    seed: int = 21, size: int = 300_000, *, min_ins: int = MIN_INS, max_ins: int = MAX_INS, frag_l: int = FRAG_L,
                    insert_mean: float = 300, insert_sd: float = 30, ragged_patl=(60, 120), random_qual: bool = False):
    """(genome, mate batch 1, mate batch 2, {category: [fragment indices planted]})

    frag_l: the length of every planted fragment (min_ins <= frag_l <= max_ins, and both mates fit into it); ragged_patl:
    one length pair, or a list of them, for the ragged part.  random_qual: the qualities of the sampled reads are drawn
    uniformly in 0..63 per base instead of 35 / 9; the PLANTED reads keep quality 35 at every base, because categories C
    and D are built on mismatch counts: with one quality everywhere the pair with fewer mismatches is also the pair
    with the better score, which is what makes D "better" and C a tie with scores on."""
    from real_amd import synth
    MAX_INS, FRAG_L = max_ins, frag_l                                  # (the planting below is written in these names)
    assert min_ins <= frag_l <= max_ins
    families = (2, 2, 3) if kind == "iid" else (2, 3, 6, 30, 60)
    g, copies = synth.repeat_family_genome(size, seed, families=families, seg_len=SEG_LEN)
    kw = dict(insert_min=min_ins, insert_max=max_ins, copies=copies, seg_len=SEG_LEN, repeat_frac=0.1 if kind == "iid" else 0.3)
    p1 = synth.sample_pairs(g, n, patl[0], patl[1], insert_mean, insert_sd, errprob, seed + 3, **dict(kw, insert_min=max(min_ins, *patl)))
    if ragged:
        p2 = ragged_parts(synth, g, n // 2, ragged_patl, insert_mean, insert_sd, errprob, seed + 4, kw)
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
    taken = set()
    for j, i in enumerate(slots):
        cat = "ABCD"[j % 4]
        X, xfwd = COMBOS[(j // 4) % 4]
        while i in taken or not (int(lens[X][i]) >= seedl + 3 and int(lens[1 - X][i]) >= seedl + totalkmax):
            i += 1                                                      # (a ragged batch may hold mates too short to plant on: the next one)
        taken.add(i)
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
    used = taken
    for b, every in ((b1, 97), (b2, 131)):                          # reads the matcher skips: a symbol > 3
        for i in range(5, b.n_reads, every):
            if i not in used:
                b.bases[int(b.offsets[i]) + 7] = 4
    if random_qual:
        random_qualities((b1, b2), sorted(taken), seed + 6)
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


# ---- real protocol shapes ----------------------------------------------------------------------------------------------
# reads, seed length, table kind asked for / prefix bits / layout built, totalkmax, insert bounds, planted fragment length,
# insert mean / sd, the ragged part's length pairs, the rescue loci of pairs_workloads (span, gap)
ProtocolRow = namedtuple("ProtocolRow", "name patl seedl tkind pb layout tk min_ins max_ins frag_l mean sd ragged_patl rescue_span rescue_gap")
EVERY_WIDTH = ((36, 320), (320, 40), (64, 288), (288, 65), (96, 256), (255, 97), (128, 192), (192, 127), (224, 160), (150, 33 + 32))
PROTOCOL_ROWS = [
    ProtocolRow("2x150_l64_rows_wide", (150, 150), 64, 3, 15, "rows", 5, 200, 700, 400, 400, 50, None, 210, 250),
    ProtocolRow("2x150_l64_fingerprint", (150, 150), 64, 2, 15, "fingerprint", 5, 200, 700, 400, 400, 50, None, 210, 250),
    ProtocolRow("2x250_l32_starts", (250, 250), 32, 0, 0, "starts", 8, 300, 900, 600, 600, 60, None, 310, 350),
    ProtocolRow("128+96_l16_rows", (128, 96), 16, 3, 13, "rows", 3, 150, 420, 300, 300, 30, None, 160, 200),
    ProtocolRow("ragged_36..320_l32_starts", (160, 224), 32, 0, 0, "starts", 5, 150, 1000, 420, 450, 100, EVERY_WIDTH, 330, 380),
]
PROTOCOL_N, PROTOCOL_SIZE = 600, 400_000
_PROTOCOL = {}


def protocol_search_workload(row: ProtocolRow, kind: str):
    """search_workload at the row's geometry (about 600 fragments, random qualities); made once, shared and never changed"""
    key = ("search", row.name, kind)
    if key not in _PROTOCOL:
        ragged = row.ragged_patl is not None
        n = 400 if ragged else PROTOCOL_N                              # (the ragged part adds n / 2)
        _PROTOCOL[key] = search_workload(kind, ragged, row.patl, row.seedl, row.tk, n=n, size=PROTOCOL_SIZE, min_ins=row.min_ins, max_ins=row.max_ins,
                                         frag_l=row.frag_l, insert_mean=row.mean, insert_sd=row.sd, ragged_patl=row.ragged_patl or (60, 120),
                                         random_qual=True)
    return _PROTOCOL[key]


def protocol_pair_workload(row: ProtocolRow, kind: str):
    """pairs_workloads.pair_workload at the row's geometry; made once, shared and never changed"""
    import pairs_workloads as pw
    key = ("pairs", row.name, kind)
    if key not in _PROTOCOL:
        ragged = row.ragged_patl is not None
        n = 400 if ragged else PROTOCOL_N
        _PROTOCOL[key] = pw.pair_workload(kind, ragged, row.patl, n=n, size=PROTOCOL_SIZE, min_ins=row.min_ins, max_ins=row.max_ins, insert_mean=row.mean,
                                          insert_sd=row.sd, ragged_patl=row.ragged_patl or (60, 120), rescue_span=row.rescue_span,
                                          rescue_gap=row.rescue_gap, random_qual=True)
    return _PROTOCOL[key]
