"""Workloads the gap rescue tests share (CPU test, GPU tests, CLI test) -- TEST INFRASTRUCTURE ONLY.

synth.sample_pairs fragments on a genome of about 100 kbp, and planted fragments whose target mate carries what the stage is
for.  A planted fragment is built from the text: the anchor mate is an exact copy, the target mate (length `patl`, the
anchor's is ANCHOR_L) gets one of
  D  a deletion of 1, 2, G - 1 or G text bases                                   -> Unique, g > 0
  I  an insertion of as many read bases                                          -> Unique, g < 0
  H  an indel of one unit inside a homopolymer or a 2-base tandem run (written into the text), taken out / put in at the
     run's END                                                                   -> the leftmost split wins: the run's start
  U  three substitutions inside the first seedl bases and no gap                 -> g = 0 beats every gapped alignment
  R  a deletion, and the target's locus copied to a second place of the window   -> NonUnique
  N  a deletion, and an N of the text inside the span                            -> NoMatch
  E  a deletion, the target lying at the very start / the very end of a text fragment -> Unique, the window is clipped
Every class cycles through target = mate 1 / mate 2 and target forward / reverse, and the indel through the split offsets
min_flank, 31, 32, 33, 64 and L - min_flank (the word boundaries of the masks and the ends of the allowed range).
The workload is a function of its arguments alone.
"""
from __future__ import annotations

import numpy as np

import gap_checker as gc

MIN_INS, MAX_INS, FRAG_L, ANCHOR_L = 150, 420, 260, 100
PER_CLASS = 8
CLASSES = "DIHURNE"
COMBOS = [(0, True), (1, True), (0, False), (1, False)]        # (the target mate, the target is the forward mate)
SEEDL, TOTALKMAX = 32, 3


class Batch:
    """a ragged batch of reads: what synth.ReadBatch holds of it"""
    def __init__(self, reads, ids=None, qual=None):
        """qual: None (35 per base), a callable length -> the qualities of one read, asked read by read, or the concatenated array"""
        self.bases = np.concatenate(reads).astype(np.uint8) if reads else np.zeros(0, np.uint8)
        if qual is None:
            self.qual = np.full(self.bases.shape[0], 35, dtype=np.uint8)
        elif callable(qual):
            self.qual = np.concatenate([qual(len(r)) for r in reads]).astype(np.uint8) if reads else np.zeros(0, np.uint8)
        else:
            self.qual = np.ascontiguousarray(qual, dtype=np.uint8)
            assert self.qual.shape == self.bases.shape
        self.offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
        self.ids = ids

    @property
    def n_reads(self):
        return int(self.offsets.shape[0]) - 1

    def read(self, i):
        return self.bases[int(self.offsets[i]):int(self.offsets[i + 1])]

    def part(self, lo, hi):
        return Batch([self.read(i) for i in range(lo, hi)], None if self.ids is None else self.ids[lo:hi],
                     self.qual[int(self.offsets[lo]):int(self.offsets[hi])])


def split_offsets(patl, prm):
    return sorted({j for j in (prm.min_flank, 31, 32, 33, 64, patl - prm.min_flank) if prm.min_flank <= j <= patl - prm.min_flank})


def gap_lengths(prm):
    return sorted({g for g in (1, 2, prm.max_gap - 1, prm.max_gap) if g >= 1})


def workload(seed=1, patl=100, prm=None, n=250, size=100_000, min_ins=MIN_INS, max_ins=MAX_INS, frag_l=None, per_class=PER_CLASS, fileid=0,
             seedl=SEEDL, anchor_l=ANCHOR_L, qual=None, n_frag=8, n_runs=6):
    """{g: synth.Genome, b1, b2: Batch, plants: [dict], prm, min_ins, max_ins}; seedl: the seed length of the run (class U puts
    its substitutions inside the first seed), anchor_l: the anchor mate's length, qual: Batch's quality generator (mate 1's
    batch is asked first), n_frag / n_runs: the text's fragments and N runs"""
    from real_amd import synth
    prm = prm or gc.default_params(TOTALKMAX)
    G, m = prm.max_gap, prm.min_flank
    frag_l = frag_l or max(FRAG_L, min_ins, patl + anchor_l + 20)
    assert min_ins <= frag_l <= max_ins and patl + anchor_l <= frag_l
    rng = np.random.default_rng(seed)
    g = synth.random_genome(size, seed + 11, n_frag=n_frag, n_runs=n_runs)
    sym, fstart = g.sym, [int(x) for x in g.frag_start]
    busy = sym > 3
    for c in fstart:
        busy[max(0, c - 1):c + 1] = True
    pad = patl + 2 * G + 40                                            # room for the copy of class R on either side

    def free_spot(length):
        for _ in range(20_000):
            s = int(rng.integers(pad, size - length - pad))
            if not busy[s - pad:s + length + pad].any():
                busy[s - pad:s + length + pad] = True
                return s
        raise RuntimeError("no free spot")

    def frag_of(x):
        return int(np.searchsorted(np.asarray(fstart), x, side="right")) - 1

    splits, gaps = split_offsets(patl, prm), gap_lengths(prm)
    plants, reads1, reads2 = [], [], []
    edge_frags = [f for f in range(len(fstart) - 1) if fstart[f + 1] - fstart[f] > 4 * frag_l]
    for j, cls in enumerate(CLASSES * per_class):
        rnd = j // len(CLASSES)
        tm, tfwd = COMBOS[(rnd + CLASSES.index(cls)) % 4]
        glen = gaps[(rnd + CLASSES.index(cls)) % len(gaps)]
        if patl < 2 * m + G + 1 or patl > gc.MAX_PATL:
            cls_eff = "S"                                                  # a target the stage skips: plain exact mates
        else:
            cls_eff = cls
        deletion = (rnd // 2 + CLASSES.index(cls)) % 2 == 0 if cls in "HRNE" else cls == "D"
        if cls_eff == "E":                                              # the target at the start (forward) / the end (reverse) of a text fragment
            f = edge_frags[rnd % len(edge_frags)]
            tfwd = rnd % 2 == 0
            tm = (rnd // 2) % 2
            span = patl + (glen if deletion else -glen)
            s = fstart[f] if tfwd else fstart[f + 1] - frag_l
            if busy[s + 2:s + frag_l - 2].any():
                continue
            busy[s:s + frag_l + pad] = True
            busy[max(0, s - pad):s] = True
        else:
            s = free_spot(frag_l)
        span = patl + (glen if deletion else -glen) if cls_eff in "DIHRNE" else patl
        xs = s if tfwd else s + frag_l - span                           # the target's footprint [xs, xs + span)
        ys = s + frag_l - anchor_l if tfwd else s                        # the anchor's
        split = splits[rnd % len(splits)]
        if not deletion:
            split = min(split, patl - m - glen)
        plant = dict(cls=cls_eff, tm=tm, tfwd=tfwd, xs=xs, span=span, frag=frag_of(xs), g=0, split=0)
        if cls_eff == "H":                                              # the run goes into the text first
            unit = np.array([0], np.uint8) if rnd % 2 == 0 else np.array([0, 1], np.uint8)
            glen = len(unit)
            span = patl + (glen if deletion else -glen)
            xs = s if tfwd else s + frag_l - span
            reps = 4
            rs = xs + max(m, min(split, patl - m - glen * (reps + 1)))  # the run's start
            sym[rs:rs + glen * reps] = np.tile(unit, reps)
            sym[rs - 1], sym[rs + glen * reps] = 2, 3                     # G in front, T behind: the run ends where it ends
            plant.update(xs=xs, span=span, run=rs)
            split = rs - xs + glen * (reps - 1) if deletion else rs - xs + glen * reps   # the indel at the run's END
        if cls_eff == "N":
            sym[xs + span // 2] = 4
        t = sym[xs:xs + span].copy()
        if cls_eff in "DHRNE" and deletion:
            r = np.concatenate([t[:split], t[split + glen:]])
            plant.update(g=glen, split=split)
        elif cls_eff in "IHRNE":
            ins = unit if cls_eff == "H" else rng.integers(0, 4, size=glen).astype(np.uint8)
            r = np.concatenate([t[:split], ins, t[split:]])
            plant.update(g=-glen, split=split)
        else:
            r = t.copy()
            if cls_eff == "S":
                r[np.arange(3, patl, max(1, patl // 7))] ^= 2             # (the matcher does not place it either)
        r[r > 3] = 1                                                    # (class N: the read shows a base where the text has none)
        assert len(r) == patl, (cls_eff, len(r), patl)
        if cls_eff == "R":                                              # the locus once more, further into the window on the side away from the anchor
            at = xs - (patl + G + 10) if tfwd else xs + (patl + G + 10)
            sym[at:at + span] = sym[xs:xs + span]
            plant.update(copy=at)
        if cls_eff == "U":
            where = rng.choice(min(seedl, patl), size=3, replace=False)
            rd = r if tfwd else gc.COMP[r[::-1]]
            rd = rd.copy()
            rd[where] ^= 2
            r = rd if tfwd else gc.COMP[rd[::-1]]
        x_read = r if tfwd else gc.COMP[r[::-1]]
        y = sym[ys:ys + anchor_l].copy()
        y_read = gc.COMP[y[::-1]] if tfwd else y
        reads1.append(x_read if tm == 0 else y_read)
        reads2.append(y_read if tm == 0 else x_read)
        plants.append(dict(plant, i=len(reads1) - 1))
    # the sampled fragments, behind the planted ones: nearly all of them are concordant pairs the stage leaves alone
    g2 = synth.Genome(sym=sym, frag_start=g.frag_start, frag_names=g.frag_names)
    bl = min(max(patl, seedl), anchor_l)
    s1, s2 = synth.sample_pairs(g2, n, bl, anchor_l, frag_l, 25, 0.02, seed + 3, insert_min=max(min_ins, anchor_l), insert_max=max_ins)
    for i in range(n):
        a, b = s1.bases[i * bl:(i + 1) * bl].copy(), s2.bases[i * anchor_l:(i + 1) * anchor_l].copy()
        if i % 41 == 7:
            a[5] = 4                                                    # a mate the matcher skips: a symbol > 3
        reads1.append(a)
        reads2.append(b)
    ids = ["f%d" % i for i in range(len(reads1))]
    return dict(g=g2, b1=Batch(reads1, [x + "/1" for x in ids], qual), b2=Batch(reads2, [x + "/2" for x in ids], qual), plants=plants, prm=prm,
                min_ins=min_ins, max_ins=max_ins, fileid=fileid, patl=patl, seedl=seedl)


def intended(plant, rec, w):
    """does the checker's record of a planted fragment show what the plant is for"""
    st, g, pos = int(gc.state_of(rec["tag"])), int(rec["gap"]), int(rec["pos"])
    cls = plant["cls"]
    right_mate = st == gc.NOMATCH or (int(gc.target_of(rec["tag"])) == plant["tm"] and int(gc.inverted_of(rec["tag"])) == (0 if plant["tfwd"] else 1))
    if not right_mate:
        return False
    if cls in "DI":
        return st == gc.UNIQUE and g == plant["g"] and pos == plant["xs"]
    if cls == "H":
        return st == gc.UNIQUE and g == plant["g"] and pos == plant["xs"] and int(rec["split"]) == plant["run"] - plant["xs"]
    if cls == "U":
        return st == gc.UNIQUE and g == 0 and int(rec["k"]) == 3 and pos == plant["xs"]
    if cls == "R":
        return st == gc.NONUNIQUE
    if cls == "N":
        return st == gc.NOMATCH
    if cls == "E":
        fs, fe = int(w["g"].frag_start[plant["frag"]]), int(w["g"].frag_start[plant["frag"] + 1])
        return st == gc.UNIQUE and g == plant["g"] and pos == plant["xs"] and (pos == fs or pos + plant["span"] == fe)
    return False


def coverage(w, rec):
    """{class: fragments that show the intended outcome}, {(target mate, forward): the same}"""
    by_class, by_combo = dict.fromkeys(CLASSES, 0), dict.fromkeys(COMBOS, 0)
    for p in w["plants"]:
        if p["cls"] in by_class and intended(p, rec[p["i"]], w):
            by_class[p["cls"]] += 1
            by_combo[(p["tm"], p["tfwd"])] += 1
    return by_class, by_combo


def oracle_records(ora, w, g=None, fileid=None, prev=None):
    """(pairs, singles1, singles2): the final records the matcher leaves for the workload's reads, from the oracle's hit lists
    through the pair and single checkers; prev: the lists of earlier genome files"""
    import pairs_checker as pc
    import singles_checker as sc
    g = g or w["g"]
    fileid = w["fileid"] if fileid is None else fileid
    b1, b2 = w["b1"], w["b2"]
    og = ora.Genome(g.sym, g.frag_start)
    ix = ora.Index(og, SEEDL)
    p = ora.make_params(seedl=SEEDL, seedkmax=2, totalkmax=TOTALKMAX, scores=False, filter_level=0, fileid=fileid)
    h1, o1, _ = ora.match_all(og, ix, p, b1.bases, b1.qual, b1.offsets)
    h2, o2, _ = ora.match_all(og, ix, p, b2.bases, b2.qual, b2.offsets)
    files = (prev or []) + [(fileid, h1, o1, h2, o2)]
    l1, l2 = np.diff(b1.offsets.astype(np.int64)), np.diff(b2.offsets.astype(np.int64))
    fm = ora.filter_mult(0, TOTALKMAX)
    pairs = pc.check_pairs(files, l1, l2, w["min_ins"], w["max_ins"], False, fm)
    sg1 = sc.check_singles([(f[0], f[1], f[2]) for f in files], l1, False, fm)
    sg2 = sc.check_singles([(f[0], f[3], f[4]) for f in files], l2, False, fm)
    return pairs, sg1, sg2, files
