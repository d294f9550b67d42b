"""Workloads the anchored gap placement tests share (CPU test, GPU tests, CLI test) -- TEST INFRASTRUCTURE ONLY.

Single-end reads on a seeded text of 100 k - 200 k bases: planted reads that carry what the stage is for, then sampled reads
the matcher places itself.  A planted read is built from the text piece [xs, xs + span):
  D  a deletion of 1 .. G text bases                                             -> Unique, g > 0
  I  an insertion of as many read bases                                          -> Unique, g < 0
  H  an indel of one unit inside a homopolymer or a 2-base tandem run (written into the text), taken out / put in at the
     run's END                                                                   -> the leftmost split wins: the run's start
  U  no gap, five substitutions (more than -e) inside one half, the other clean  -> Unique, g = 0, k = 5
  R  an indel, and the locus copied to a second place                            -> NonUnique
  P  an indel min_flank bases behind the read's start: inside the prefix sub-read, only the suffix anchors it
  S  an indel min_flank bases in front of its end: inside the suffix sub-read, only the prefix anchors it
  E  an insertion in a read that starts at the very start of a text fragment (the tail anchor's diagonal lies in front of
     the fragment; in fragment 0 it is negative), or a deletion in one that ends at its very end
  N  an indel, and an N of the text in the middle of the span                    -> NoMatch
  C  a deletion, the locus copied COPIES more times: both sub-reads hit every copy  -> crowded
Every class cycles through the strands, the gap lengths 1 .. G and (D, I, R) the split offsets min_flank, 31, 32, 33, 64 and
L - min_flank.  Behind the plants: sampled reads with 2 % substitutions (the matcher places nearly all: not eligible), every
41st with a symbol > 3 (skipped).  The workload is a function of its arguments alone.
"""
from __future__ import annotations

import numpy as np

import gap_checker as gc
from gap_workloads import Batch, split_offsets

CLASSES = "DIHURPSENC"
PER_CLASS = 8
COPIES = 40
TOTALKMAX = 3


def seedl_of(patl):
    """the seed length of the index a read length is tested with: a sub-read is at least a seed"""
    return 12 if patl <= 33 else 16 if patl <= 65 else 32


def default_anchor(patl, prm):
    """(L - G) / 2: the longest anchor with full coverage, 2 A + G <= L"""
    return (patl - prm.max_gap) // 2


def default_params(patl=100, **kw):
    return gc.default_params(1 if patl <= 33 else TOTALKMAX, **kw)


def workload(seed=1, patl=100, prm=None, n=150, size=150_000, per_class=PER_CLASS, fileid=0, classes=CLASSES,
             seedl=None, qual=None, n_frag=6, n_runs=4):
    """{g: synth.Genome, b: Batch, plants: [dict], prm, patl, fileid, seedl}; seedl: the seed length of the run (None: seedl_of
    the read length), qual: Batch's quality generator, n_frag / n_runs: the text's fragments and N runs"""
    from real_amd import synth
    prm = prm or default_params(patl)
    G, m = prm.max_gap, prm.min_flank
    rng = np.random.default_rng(seed)
    g = synth.random_genome(size, seed + 11, n_frag=n_frag, n_runs=n_runs)
    sym, fstart = g.sym, [int(x) for x in g.frag_start]
    busy = sym > 3
    for c in fstart[1:-1]:
        busy[max(0, c - 1):c + 1] = True
    pad = 2 * G + 8
    edge = patl + G + pad                                                   # both ends of every fragment are kept for class E
    for f in range(len(fstart) - 1):
        if fstart[f + 1] - fstart[f] >= 2 * edge:
            busy[fstart[f]:fstart[f] + edge] = True
            busy[fstart[f + 1] - edge:fstart[f + 1]] = True
    searched = 2 * m + G + 1 <= patl <= gc.MAX_PATL

    def free_spot(length):
        for _ in range(20_000):
            s = int(rng.integers(pad + 1, size - length - pad - 1))
            if not busy[s - pad:s + length + pad].any():
                busy[s - pad:s + length + pad] = True
                return s
        raise RuntimeError("no free spot")

    def frag_of(x):
        return int(np.searchsorted(np.asarray(fstart), x, side="right")) - 1

    splits = split_offsets(patl, prm) if searched else [patl // 2]
    plants, reads = [], []
    n_frag = len(fstart) - 1
    for j, cls in enumerate(classes * per_class):
        rnd, ci = j // len(classes), classes.index(cls)
        fwd = (rnd + ci) % 2 == 0
        glen = G - (rnd + ci) % G
        deletion = cls == "D" or (cls in "HRPSNC" and (rnd // 2 + ci) % 2 == 0) or cls == "C"
        if cls == "E":
            at_start = (rnd // 2) % 2 == 0
            deletion = not at_start
        if not searched:
            cls, glen, deletion = "X", 1, True                              # a read the stage skips (too short, too long)
        span = patl + (glen if deletion else -glen) if cls != "U" else patl
        if cls == "E":
            f = rnd % n_frag
            xs = fstart[f] if at_start else fstart[f + 1] - span
            if fstart[f + 1] - fstart[f] < 2 * edge or (sym[xs:xs + span] > 3).any():
                continue
        else:
            xs = free_spot(span)
        split = splits[rnd % len(splits)] if cls in "DIRX" else m if cls == "P" else patl - m if cls == "S" else patl // 2
        if not deletion:
            split = min(split, patl - m - glen)
        plant = dict(cls=cls, fwd=fwd, xs=xs, span=span, frag=frag_of(xs), g=0, split=0)
        if cls == "H":                                                      # the run goes into the text first
            unit = np.array([0], np.uint8) if rnd % 2 == 0 else np.array([0, 1], np.uint8)
            glen, reps = len(unit), 4
            span = patl + (glen if deletion else -glen)
            rs = xs + max(m, min(splits[rnd % len(splits)], patl - m - glen * (reps + 1)))   # the run's start
            sym[rs:rs + glen * reps] = np.tile(unit, reps)
            sym[rs - 1], sym[rs + glen * reps] = 2, 3                         # G in front, T behind: the run ends where it ends
            plant.update(span=span, run=rs)
            split = rs - xs + glen * (reps - 1) if deletion else rs - xs + glen * reps       # the indel at the run's END
        if cls == "N":
            sym[xs + span // 2] = 4
        t = sym[xs:xs + span].copy()
        if cls == "U":
            r = t.copy()
            half = (rnd // 2) % 2                                           # which half carries the substitutions
            where = rng.choice(np.arange(patl // 2 + 2, patl - 1) if half else np.arange(1, patl // 2 - 2), size=5, replace=False)
            r[where] ^= 2
            plant.update(half=half)
        elif deletion:
            r = np.concatenate([t[:split], t[split + glen:]])
            plant.update(g=glen, split=split)
        else:
            ins = unit if cls == "H" else rng.integers(0, 4, size=glen).astype(np.uint8)
            r = np.concatenate([t[:split], ins, t[split:]])
            plant.update(g=-glen, split=split)
        r[r > 3] = 1                                                        # (class N: the read shows a base where the text has none)
        assert len(r) == patl, (cls, len(r), patl)
        if cls == "R":
            at = free_spot(span)
            sym[at:at + span] = sym[xs:xs + span]
            plant.update(copy=at)
        if cls == "C":
            for _ in range(COPIES):
                at = free_spot(span)
                sym[at:at + span] = sym[xs:xs + span]
        reads.append(r if fwd else gc.COMP[r[::-1]])
        plants.append(dict(plant, i=len(reads) - 1))
    g2 = synth.Genome(sym=sym, frag_start=g.frag_start, frag_names=g.frag_names)
    bl = min(patl, gc.MAX_PATL)
    sampled = synth.sample_reads(g2, n, bl, 0.02, seed + 3)
    for i in range(n):
        a = sampled.bases[i * bl:(i + 1) * bl].copy()
        if i % 41 == 7:
            a[5] = 4                                                        # a read the matcher and the stage skip: a symbol > 3
        reads.append(a)
    ids = ["r%d" % i for i in range(len(reads))]
    return dict(g=g2, b=Batch(reads, ids, qual), plants=plants, prm=prm, patl=patl, fileid=fileid, seedl=seedl or seedl_of(patl))


def intended(plant, rec, w):
    """does the checker's record of a planted read show what the plant is for"""
    st, g, pos = int(gc.state_of(rec["tag"])), int(rec["gap"]), int(rec["pos"])
    cls = plant["cls"]
    if st != gc.NOMATCH and int(gc.inverted_of(rec["tag"])) != (0 if plant["fwd"] else 1):
        return False
    if cls in "DIPS":
        return st == gc.UNIQUE and g == plant["g"] and pos == plant["xs"]
    if cls == "H":
        return st == gc.UNIQUE and g == plant["g"] and pos == plant["xs"] and int(rec["split"]) == plant["run"] - plant["xs"]
    if cls == "U":
        return st == gc.UNIQUE and g == 0 and int(rec["k"]) == 5 and pos == plant["xs"]
    if cls == "R":
        return st == gc.NONUNIQUE
    if cls in "NC":
        return st == gc.NOMATCH
    if cls == "E":
        fs, fe = int(w["g"].frag_start[plant["frag"]]), int(w["g"].frag_start[plant["frag"] + 1])
        return st == gc.UNIQUE and g == plant["g"] and pos == plant["xs"] and (pos == fs or pos + plant["span"] == fe)
    return False


def coverage(w, rec):
    """{class: reads that show the intended outcome}, {forward: the same}"""
    by_class, by_strand = dict.fromkeys(CLASSES, 0), {True: 0, False: 0}
    for p in w["plants"]:
        if p["cls"] in by_class and intended(p, rec[p["i"]], w):
            by_class[p["cls"]] += 1
            by_strand[p["fwd"]] += 1
    return by_class, by_strand


def oracle_lists(ora, w, a_len, g=None, fileid=None, first_window=0, max_entries=1 << 62, totalkmax=None):
    """(info, hits, hit offsets): the oracle's final info words of the workload's reads and its matchAll lists of S(b, A)"""
    import gap_anchor_checker as gac
    g = g or w["g"]
    fileid = w["fileid"] if fileid is None else fileid
    e = (1 if w["patl"] <= 33 else TOTALKMAX) if totalkmax is None else totalkmax
    og = ora.Genome(g.sym, g.frag_start)
    ix = ora.Index(og, w["seedl"], first_window, max_entries)
    p = ora.make_params(seedl=w["seedl"], seedkmax=min(2, e), totalkmax=e, scores=False, filter_level=0, fileid=fileid)
    b = w["b"]
    info, _, _ = ora.match_unique(og, ix, p, b.bases, b.qual, b.offsets)
    sub = gac.SubBatch(b, a_len)
    hits, hoff, _ = ora.match_all(og, ix, p, sub.bases, sub.qual, sub.offsets)
    return info, hits, hoff


def oracle_run(ora, w, a_len, genomes, per_block=1 << 62, totalkmax=TOTALKMAX):
    """A run of the command line over the genome files [(genome, fileid)], index blocks of per_block entries: the oracle's
    final info words, and per index block, in the run's order, (fileid, genome, hits, hit offsets) of its matchAll of S(b, A)"""
    import gap_anchor_checker as gac
    b = w["b"]
    sub = gac.SubBatch(b, a_len)
    info, blocks = None, []
    for g, fid in genomes:
        og = ora.Genome(g.sym, g.frag_start)
        p = ora.make_params(seedl=w["seedl"], seedkmax=2, totalkmax=totalkmax, scores=False, filter_level=0, fileid=fid)
        first = 0
        while True:
            ix = ora.Index(og, w["seedl"], first, per_block)
            info, _, _ = ora.match_unique(og, ix, p, b.bases, b.qual, b.offsets, info=info)
            hits, hoff, _ = ora.match_all(og, ix, p, sub.bases, sub.qual, sub.offsets)
            blocks.append((fid, g, hits, hoff))
            first += ix.n
            if not ix.have_next:
                break
    return info, blocks
