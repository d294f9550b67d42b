"""Workloads of the indel call tests (CPU test, GPU test) -- TEST INFRASTRUCTURE ONLY.

hand_cases()  gap records and pair records written by hand over a text of its own -- no matcher and no rescue behind them: the
              splits, gap lengths, read lengths, mates and strands the add kernel takes another path at; homopolymer and
              dinucleotide runs whose left shift crosses word boundaries, ends at a fragment's first base plus one, ends in
              front of an N, ends exactly at the cap and beyond it; an anchor at n - 2; N bits at an anchor and inside a deleted
              range; groups of 1, 2, 64, 65 and 300 mates; qualities on both sides of 20; the hand table of the header; and the
              records that must give nothing.  The pair records place ungapped mates over some loci: the depth beside the events.
planted()     a two-haplotype workload in the style of call_workloads.py: homozygous and heterozygous insertions and deletions
              of 1 .. 8 bases, fragments of 2 x 100 bases cut from the haplotypes in turn at a mean depth of about 30.
Both are functions of their arguments.
"""
from __future__ import annotations

import functools
import types

import numpy as np

import gap_checker as gc
import gap_workloads as gw
import pileup_checker as pk

HAND_N = 40_000 + 13                      # no multiple of 32 or 64
HAND_CUT = 17_001                         # the second fragment's first base
N_RUN = (9_000, 9_040)
SPLITS = (1, 31, 32, 33, 64)
GAPS = (-16, -15, -1, 1, 16)
LENGTHS = (25, 100, 320)
PAIR_DTYPE = np.dtype([("best", "<f8"), ("second", "<f8"), ("pos1", "<u4"), ("pos2", "<u4"), ("score1", "<f4"), ("score2", "<f4"),
                       ("frag", "<u2"), ("fileid", "u1"), ("k1", "u1"), ("k2", "u1"), ("inverted1", "u1"), ("state", "u1"),
                       ("reserved", "u1")])
EMPTY_NOTES = {"NoMatch": None, "NonUnique": None, "other file": "other_file", "pos + span = n + 1": "invalid", "split 0 with a gap": "invalid",
               "split + d = L": "invalid", "gap 17": "invalid", "gap -17": "invalid", "ungapped with a split": "invalid",
               "a read of 321 bases with a gap": "invalid", "a fragment the text has not": "invalid", "the other fragment": "invalid",
               "a span across the fragments": "invalid", "ungapped": "ungapped", "N at the anchor": "on_n", "N in the deleted range": "on_n"}


class Batch(gw.Batch):
    """gap_workloads.Batch with qualities of its own (None: a batch without)"""
    def __init__(self, reads, quals=None, ids=None):
        super().__init__(reads, ids)
        self._quals = quals
        self.qual = None if quals is None else (np.concatenate(quals).astype(np.uint8) if quals else np.zeros(0, np.uint8))

    def part(self, lo, hi):
        return Batch([self.read(i) for i in range(lo, hi)], None if self._quals is None else self._quals[lo:hi], None if self.ids is None else self.ids[lo:hi])

    def without_qualities(self):
        return Batch([self.read(i) for i in range(self.n_reads)], None, self.ids)


def hand_cases(seed=5, fileid=0):
    """{sym, frag_start, b1, b2, gaps, what: [str], pb1, pb2, pairs, table: {name: anchor}, fileid}"""
    rng = np.random.default_rng(seed)
    n = HAND_N
    sym = rng.integers(0, 4, size=n).astype(np.uint8)
    frag_start = [0, HAND_CUT, n]
    sym[N_RUN[0]:N_RUN[1]] = 4

    def run(at, unit, length, before=None):
        """a tandem run of `unit` over [at, at + length), another base in front of it and behind it"""
        u = np.array(unit, dtype=np.uint8)
        sym[at:at + length] = np.resize(u, length)
        if before is not False and at > 0:
            sym[at - 1] = (u[-1] + 1) & 3 if before is None else before
        sym[at + length] = (sym[at + length - len(u)] + 2) & 3
    run(2_030, [0], 50)                    # a homopolymer over the word boundary 2048 = 64 * 32
    run(3_000, [1, 2], 60)                 # a dinucleotide run over 3008 = 94 * 32 and 3040
    run(HAND_CUT, [3], 29, before=False)   # a homopolymer from the second fragment's first base on
    sym[HAND_CUT - 1] = 3                  # (the same base in front of the fragment: only the fragment's start stops the shift)
    sym[5_000] = 4
    run(5_001, [2], 39, before=False)      # a homopolymer behind an N
    run(6_000, [1], 400)                   # longer than the cap
    run(7_000, [0], 257)                   # 256 shifts exactly: the cap is reached and is not what stops the event
    run(7_500, [3, 0], 300)                # a dinucleotide run longer than the cap
    sym[11_000], sym[11_300 + 3] = 4, 4    # an N at an anchor, an N inside a deleted range
    table = {"10/10": 24_000, "12/0": 25_000, "1/20": 26_000, "3/3": 27_000}   # the hand table's loci: nothing shifts there
    for name, x in table.items():
        sym[x - 1] = 1 if name == "12/0" else (sym[x + 1] + 1) & 3
    src = np.where(sym > 3, 1, sym).astype(np.uint8)
    reads1, reads2, q1, q2, recs, what = [], [], [], [], [], []

    def frag_of(x):
        return int(np.searchsorted(np.asarray(frag_start), x, side="right")) - 1

    def add(x, g, l, j, tm, inv, s=None, qual=35, state=gc.UNIQUE, file=fileid, frag=None, pos=None, note=""):
        """a mate of l bases that shows the event (x, g, S = s) at split j: its placement starts at x - j"""
        d, dele = max(-g, 0), max(g, 0)
        p = x - j if pos is None else pos
        span = l + g
        c = max(0, min(p, n - span))                                     # (records that do not fit: any l bases of the text)
        ins = np.asarray(rng.integers(0, 4, size=d) if s is None else s, dtype=np.uint8)
        o = np.concatenate([src[c:c + j], ins, src[c + j + dele:c + span]]) if g else src[c:c + l].copy()
        o = np.resize(o, l).astype(np.uint8)
        qo = np.full(l, 35, dtype=np.uint8)
        if isinstance(qual, dict):                                       # {oriented offset relative to j: quality}
            for k, v in qual.items():
                qo[j + k] = v
        else:
            qo[:] = qual
        read, qr = (gc.COMP[o[::-1]], qo[::-1]) if inv else (o, qo)
        other, qother = rng.integers(0, 4, size=30).astype(np.uint8), np.full(30, 35, dtype=np.uint8)
        reads1.append(read if tm == 0 else other)
        reads2.append(other if tm == 0 else read)
        q1.append(qr if tm == 0 else qother)
        q2.append(qother if tm == 0 else qr)
        r = gc.empty_records(1)[0]
        r["pos"], r["frag"], r["fileid"], r["split"], r["gap"], r["k"], r["cost"] = p & 0xffffffff, frag_of(x) if frag is None else frag, file, j, g, 0, 7
        r["tag"] = tm | (inv << 4) | (state << 5)
        recs.append(r)
        what.append(note or "x%d g%d L%d j%d" % (x, g, l, j))

    # every split, gap and read length, each event shown once; mates and strands in turn
    turn, x = 0, 12_000
    for l in LENGTHS:
        for g in GAPS:
            d = max(-g, 0)
            for j in sorted({*SPLITS, l - 1 - d}):
                if not (1 <= j and j + d <= l - 1):
                    continue
                add(x, g, l, j, turn & 1, (turn >> 1) & 1)
                turn += 1
                x += 61 if x < HAND_CUT - 800 or x > HAND_CUT + 400 else 1_200       # (none across the fragments' border)
    assert x < n - 400
    # one event shown by both mates on both strands, at other splits and lengths: the same S whatever the orientation
    s7 = [0, 3, 1, 1, 2, 0, 3]
    for k, (tm, inv) in enumerate(gw.COMBOS * 2):
        add(1_000, -7, (100, 80)[k & 1], 20 + 7 * k, tm, int(not inv), s=s7)
        add(1_300, 5, (100, 64)[k & 1], 11 + 5 * k, tm, int(not inv))
    # two insertions of equal position and length but other bases; a deletion and an insertion at one anchor
    for k in range(3):
        add(1_600, -3, 100, 30 + k, k & 1, 0, s=[0, 1, 3])
        add(1_600, -3, 100, 50 + k, k & 1, 1, s=[0, 2, 3])
        add(1_600, 3, 100, 40 + k, 1, k & 1)
    # the runs: the event at the run's end and inside it, as a deletion and an insertion of one unit
    for at, unit, length, j0 in ((2_030, [0], 50, 40), (3_000, [1, 2], 60, 40), (HAND_CUT, [3], 29, 3), (5_001, [2], 39, 40), (6_000, [1], 400, 40),
                                 (7_000, [0], 257, 40), (7_500, [3, 0], 300, 40)):
        u = len(unit)
        end, mid = at + length, at + length // 2 + 1
        tail = [int(v) for v in sym[end - u:end]]
        for k in range(4):
            add(end - u, u, 100, j0 + k, k & 1, k >> 1)                 # the last unit deleted
            add(end, -u, 100, j0 + 5 + k, k >> 1, k & 1, s=tail)        # one more unit behind the run
        add(mid, u, 100, min(33, j0 + 2), 0, 0)                         # from the middle of the run
        add(mid, -u, 100, min(64, j0 + 4), 1, 1, s=[int(v) for v in sym[mid - u:mid]])
    # an anchor at n - 2: an insertion in front of the text's last base; and one in front of the first fragment's second base
    add(n - 1, -4, 100, 95, 0, 0)
    add(n - 1, -4, 64, 59, 1, 1)
    add(1, -2, 50, 1, 0, 1)
    add(1, 2, 50, 1, 1, 0)
    # N bits
    add(11_001, 2, 100, 40, 0, 0, note="N at the anchor")
    add(11_001, -2, 100, 40, 1, 1, note="N at the anchor")
    add(11_300, 6, 100, 50, 0, 1, note="N in the deleted range")
    add(11_305, -6, 100, 50, 0, 1)                                      # (an N in front of the anchor drops nothing, and stops the shift)
    # the group sizes: 1 and 2 are above; 64, 65 and 300 mates, lengths, splits, mates and strands in turn
    for x0, g, size in ((20_000, 2, 64), (20_600, -2, 65), (21_200, 4, 300)):
        s = [1, 3] if g < 0 else None
        for k in range(size):
            add(x0, g, (100, 64, 150)[k % 3], 10 + k % 47, k & 1, (k >> 1) & 1, s=s)
    # qualities on both sides of 20, at each offset the minimum is taken over
    for k, off in enumerate((-1, 0, 1, 2, 3)):
        add(22_000, -3, 100, 30 + k, k & 1, k >> 2, s=[2, 2, 1], qual={off: 19})           # j - 1 .. j + d = j + 3
        add(22_000, -3, 100, 40 + k, k & 1, k >> 2, s=[2, 2, 1], qual={off: 20})
    add(22_000, -3, 100, 20, 0, 1, s=[2, 2, 1], qual={-2: 3, 4: 3})                        # (outside the offsets: it counts)
    for k, off in enumerate((-1, 0)):
        add(22_400, 3, 100, 30 + k, k & 1, 1, qual={off: 19})
        add(22_400, 3, 100, 40 + k, k & 1, 0, qual={off: 21})
    add(22_400, 3, 100, 50, 0, 0, qual={-2: 0, 1: 0})
    # the hand table, all q 30: alt 10 / ref 10, alt 12 / ref 0, alt 1 / ref 20 (the depth comes from the pair records below)
    for name, alt in (("10/10", 10), ("12/0", 12), ("1/20", 1), ("3/3", 3)):
        for k in range(alt):
            add(table[name], 2 if name != "12/0" else -2, 100, 30 + k, k & 1, (k >> 1) & 1, s=[0, 0], qual=30)
    add(28_000, 3, 100, 30, 0, 0)                                       # a group of two
    add(28_000, 3, 64, 50, 1, 1)
    # the records that must give nothing
    ok = dict(x=2_600, g=2, l=100, j=40, tm=0, inv=0)
    add(**ok, state=gc.NOMATCH, note="NoMatch")
    add(**ok, state=gc.NONUNIQUE, note="NonUnique")
    add(**dict(ok, tm=1), file=fileid + 1, note="other file")
    add(**ok, pos=n + 1 - 102, frag=1, note="pos + span = n + 1")
    add(**dict(ok, j=0), pos=2_560, note="split 0 with a gap")
    add(**dict(ok, g=-3, j=97, tm=1), note="split + d = L")
    add(**dict(ok, g=17), note="gap 17")
    add(**dict(ok, g=-17, inv=1), note="gap -17")
    add(**dict(ok, g=0, j=5), note="ungapped with a split")
    add(**dict(ok, l=321, g=1), note="a read of 321 bases with a gap")
    add(**ok, frag=2, note="a fragment the text has not")
    add(**ok, frag=1, note="the other fragment")
    add(**dict(ok, x=HAND_CUT + 10, j=40), frag=0, note="a span across the fragments")
    add(**dict(ok, g=0, j=0), note="ungapped")
    add(**ok, note="a fitting record behind them")
    gaps = np.array(recs, dtype=gc.REC_DTYPE)
    # the pair records: ungapped mates over the table's loci and over some of the groups -- the depth beside the events
    pr1, pr2, pq1, pq2, prec = [], [], [], [], []

    def cover(x, copies, l=100):
        for k in range(copies):
            p1 = x - 10 - (k * 7) % (l - 20)                             # covers x - 1 and x
            p2 = p1 + 150
            r = np.zeros(1, dtype=PAIR_DTYPE)[0]
            r["pos1"], r["pos2"], r["frag"], r["fileid"], r["inverted1"], r["state"] = p1, p2, frag_of(x), fileid, k & 1, pk.UNIQUE
            a, b = src[p1:p1 + l], src[p2:p2 + l]
            pr1.append(gc.COMP[a[::-1]] if k & 1 else a.copy())
            pr2.append(b.copy() if k & 1 else gc.COMP[b[::-1]])
            pq1.append(np.full(l, 30, np.uint8))
            pq2.append(np.full(l, 30, np.uint8))
            prec.append(r)
    cover(table["10/10"] - 0, 10)
    cover(table["1/20"], 20)
    cover(table["3/3"], 3)
    cover(20_000, 40)
    cover(21_200, 7)
    cover(1_600, 5)
    cover(6_000 + 120, 9)                                               # where the capped events of the long run end up
    # one side of an event covered more than the other: ref_n is the smaller depth
    for k in range(6):
        r = np.zeros(1, dtype=PAIR_DTYPE)[0]
        r["pos1"], r["pos2"], r["fileid"], r["state"] = 20_600 - 100, 20_600 + 60, fileid, pk.UNIQUE     # mate 1 ends at x - 1
        pr1.append(src[20_500:20_600].copy())
        pr2.append(gc.COMP[src[20_660:20_760][::-1]])
        pq1.append(np.full(100, 30, np.uint8))
        pq2.append(np.full(100, 30, np.uint8))
        prec.append(r)
    return dict(sym=sym, frag_start=np.array(frag_start, dtype=np.uint64), b1=Batch(reads1, q1), b2=Batch(reads2, q2), gaps=gaps, what=what,
                pb1=Batch(pr1, pq1), pb2=Batch(pr2, pq2), pairs=np.array(prec, dtype=PAIR_DTYPE), table=table, fileid=fileid)


# ---- the planted workload ------------------------------------------------------------------------------------------------------
P_SIZE, P_DEPTH, P_READ, P_FRAG_MIN, P_FRAG_MAX = 30_000, 30, 100, 260, 340
P_CLASSES = ("hom_ins", "hom_del", "het_ins", "het_del")
P_PER_CLASS = 6
SEEDL, SEEDKMAX, TOTALKMAX = gw.SEEDL, 1, 1
# -e 1: the matcher places a mate ungapped over an indel only where the indel lies in the mate's last base or two.  Such mates
# count towards ref_n, and PL(1/1) = 30 ref_n + 43 loses against PL(0/1) = 3 (ref_n + alt_n) + 40 as soon as alt_n <= 9 ref_n + 1:
# with -e 3 about a quarter of the homozygous loci have ref_n >= 3 at depth 30 and are called 0/1 (measured: 20 of 23 right).


@functools.lru_cache(maxsize=None)
def planted(seed=7):
    """-> namespace: g (the reference genome, two fragments), plants [{cls, x, g, s, hom}] (the indel as planted; planted_key() gives
    its left-normalised name), snps {position: (ref, alt, homozygous)}, b1 / b2 (the mates), min_ins, max_ins, prm (the rescue's
    parameters)"""
    from real_amd import synth
    rng = np.random.default_rng(seed)
    g = synth.random_genome(P_SIZE, seed + 1, n_frag=2, n_runs=0)
    sym = g.sym
    fstart = [int(v) for v in g.frag_start]
    assert not (sym > 3).any()
    # loci 1100 bases apart, away from the fragments' ends
    spots = [x for x in range(800, P_SIZE - 800, 1_100) if all(abs(x - c) > 700 for c in fstart)]
    plants = []
    for k, x in enumerate(spots[:P_PER_CLASS * len(P_CLASSES)]):
        cls = P_CLASSES[k % len(P_CLASSES)]
        size = 1 + (k // len(P_CLASSES) + k) % 8
        ins = "ins" in cls
        plants.append(dict(cls=cls, x=x, g=-size if ins else size, s=[int(v) for v in rng.integers(0, 4, size=size)] if ins else [], hom="hom" in cls,
                           hap=k & 1))
    # the haplotypes, as lists of (reference position, base) so that a read knows where it starts on the reference
    # substitutions half way between the loci, homozygous and heterozygous in turn: the SNP lines the indel lines are merged with
    snps = {}
    for k, p in enumerate(plants[:16]):
        x = p["x"] + 550
        snps[x] = (int(sym[x]), int((sym[x] + 1 + k % 3) & 3), k % 2 == 0)       # (ref, alt, homozygous)

    def haplotype(h):
        out, at = [], 0
        src = sym.copy()
        for k, (x, (ref, alt, hom)) in enumerate(sorted(snps.items())):
            if hom or (k >> 1) % 2 == h:
                src[x] = alt
        for p in plants:
            if not (p["hom"] or p["hap"] == h):
                continue
            out.append(src[at:p["x"]])
            if p["g"] < 0:
                out.append(np.array(p["s"], dtype=np.uint8))
                at = p["x"]
            else:
                at = p["x"] + p["g"]
        out.append(src[at:])
        return np.concatenate(out).astype(np.uint8)
    haps = [haplotype(0), haplotype(1)]
    # the fragments: cut from the haplotypes in turn, both orders of the mates, a few substitutions
    reads1, reads2, q1, q2 = [], [], [], []
    n_frag = P_DEPTH * P_SIZE // (2 * P_READ)
    for i in range(n_frag):
        hp = haps[i & 1]
        fl = int(rng.integers(P_FRAG_MIN, P_FRAG_MAX + 1))
        s = int(rng.integers(0, hp.shape[0] - fl))
        if any(s < c + 120 and s + fl > c - 120 for c in fstart[1:-1]):     # (none across the fragments' border)
            continue
        a, b = hp[s:s + P_READ].copy(), hp[s + fl - P_READ:s + fl].copy()
        for r in (a, b):
            mut = rng.random(P_READ) < 0.004
            r[mut] = (r[mut] + rng.integers(1, 4, size=int(mut.sum()))) & 3
        fwd_first = bool(rng.integers(0, 2))
        m1, m2 = (a, gc.COMP[b[::-1]]) if fwd_first else (gc.COMP[b[::-1]], a)
        reads1.append(m1)
        reads2.append(m2)
        q1.append(rng.integers(25, 41, size=P_READ).astype(np.uint8))
        q2.append(rng.integers(25, 41, size=P_READ).astype(np.uint8))
    ids = ["p%d" % i for i in range(len(reads1))]
    return types.SimpleNamespace(g=g, plants=plants, snps=snps, b1=Batch(reads1, q1, [x + "/1" for x in ids]), b2=Batch(reads2, q2, [x + "/2" for x in ids]),
                                 min_ins=P_FRAG_MIN - 20, max_ins=P_FRAG_MAX + 20, prm=gc.default_params(TOTALKMAX), fileid=0)


def oracle_records(ora, w, g=None, fileid=None, prev=None, b1=None, b2=None):
    """(pairs, singles1, singles2, files): the final records the matcher leaves for the planted workload's reads (or b1 / b2) over the
    genome g as file `fileid`, from the oracle's hit lists through the pair and single checkers (gap_workloads.oracle_records with
    this workload's -e); prev: the lists of earlier genome files"""
    import pairs_checker as pc
    import singles_checker as sc
    g = g or w.g
    fileid = w.fileid if fileid is None else fileid
    b1, b2 = b1 or w.b1, b2 or w.b2
    og = ora.Genome(g.sym, g.frag_start)
    ix = ora.Index(og, SEEDL)
    p = ora.make_params(seedl=SEEDL, seedkmax=SEEDKMAX, totalkmax=TOTALKMAX, scores=False, filter_level=0, fileid=fileid)
    h1, o1, _ = ora.match_all(og, ix, p, b1.bases, b1.qual, b1.offsets)
    h2, o2, _ = ora.match_all(og, ix, p, b2.bases, b2.qual, b2.offsets)
    files = (prev or []) + [(fileid, h1, o1, h2, o2)]
    l1, l2 = np.diff(b1.offsets.astype(np.int64)), np.diff(b2.offsets.astype(np.int64))
    fm = ora.filter_mult(0, TOTALKMAX)
    return (pc.check_pairs(files, l1, l2, w.min_ins, w.max_ins, False, fm), sc.check_singles([(f[0], f[1], f[2]) for f in files], l1, False, fm),
            sc.check_singles([(f[0], f[3], f[4]) for f in files], l2, False, fm), files)


def planted_key(w, p):
    """(anchor, g, packed S) of a planted indel as the stage names it: left-normalised against the reference"""
    import indel_checker as ic
    fs = [int(v) for v in w.g.frag_start]
    f = int(np.searchsorted(np.asarray(fs), p["x"], side="right")) - 1
    xf, s, _, _ = ic.shift_loop(w.g.sym, fs[f], p["x"], p["g"], p["s"])
    return xf - 1, p["g"], ic.pack_seq(s)
