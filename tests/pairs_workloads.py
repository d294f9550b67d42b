"""Workloads the paired-end tests share (GPU tests, CLI test), so that their seeds are tuned in one place -- TEST
INFRASTRUCTURE ONLY.  The checker itself is pairs_checker.py."""
from __future__ import annotations

import numpy as np

from pairs_checker import NOMATCH, NONUNIQUE, UNIQUE

# ---- shared workloads -----------------------------------------------------------------------------------------------
RESCUE_SPAN, RESCUE_GAP, SEG_LEN = 160, 200, 760
MIN_INS, MAX_INS = 150, 420


def pair_workload(kind: str, ragged: bool, patl=(100, 80), n: int = 1500, errprob: float = 0.01, seed: int = 11, size: int = 400_000, *,
                  min_ins: int = MIN_INS, max_ins: int = MAX_INS, insert_mean: float = 300, insert_sd: float = 30, ragged_patl=(60, 120),
                  rescue_span: int = RESCUE_SPAN, rescue_gap: int = RESCUE_GAP, random_qual: bool = False):
    """(genome, mate batch 1, mate batch 2): an i.i.d. genome with perturbed repeats or repeat_family_genome (3/6/30/60
    copies), both with loci where pairing rescues a fragment; a few reads carry an N (skipped by the matcher).

    The insert bounds, the insert mean / sd, the length pair(s) of the ragged part and the geometry of the rescue loci
    (a mate must fit into rescue_span) are arguments; the defaults give the inputs every earlier caller has always had
    (test_workload_defaults_cpu.py holds their hashes).  random_qual: per-base qualities uniform in 0..63 instead of
    35 / 9, for every read (nothing here is planted on a read, so no read needs a fixed quality)."""
    from real_amd import synth
    from mate_search_workloads import ragged_parts, random_qualities
    RESCUE_SPAN, RESCUE_GAP = rescue_span, rescue_gap
    if kind == "families":
        g, copies = synth.repeat_family_genome(size, seed, seg_len=SEG_LEN)
        avoid = [(p, p + SEG_LEN) for fam in copies for p in fam]
    else:
        g = synth.random_genome(size, seed, n_frag=4, n_runs=6, repeats=0)
        rng = np.random.default_rng(seed + 1)
        copies = []
        for _ in range(6):                                         # exact two- and three-copy segments
            at = [int(v) for v in rng.integers(1000, size - 2000, size=int(rng.integers(2, 4)))]
            for p in at[1:]:
                g.sym[p:p + SEG_LEN] = g.sym[at[0]:at[0] + SEG_LEN]
            copies.append(tuple(at))
        avoid = [(p, p + SEG_LEN) for fam in copies for p in fam]
    loci = synth.plant_pair_repeats(g, 8, RESCUE_SPAN, RESCUE_GAP, seed + 2, avoid=avoid)
    kw = dict(insert_min=min_ins, insert_max=max_ins, copies=copies, seg_len=SEG_LEN, rescue_loci=loci, rescue_span=RESCUE_SPAN,
              rescue_gap=RESCUE_GAP, rescue_frac=0.08)
    p1 = synth.sample_pairs(g, n, patl[0], patl[1], insert_mean, insert_sd, errprob, seed + 3, **dict(kw, insert_min=max(min_ins, *patl)))
    if ragged:
        p2 = ragged_parts(synth, g, n // 2, ragged_patl, insert_mean, insert_sd, errprob, seed + 4, kw)
        b1, b2 = synth.ragged_pairs(p1, p2)
    else:
        b1, b2 = p1
    for b, every in ((b1, 97), (b2, 131)):                         # reads the matcher skips: a symbol > 3
        for i in range(5, b.n_reads, every):
            b.bases[int(b.offsets[i]) + 7] = 4
    if random_qual:
        random_qualities((b1, b2), (), seed + 6)
    return g, b1, b2


def lens_of(b):
    return (b.offsets[1:] - b.offsets[:-1]).astype(np.uint32)


def oracle_pairs(ora, g, b1, b2, seedl, totalkmax, scores, filter_level, fileid=0, want_single=False):
    """the checker's records for one genome file from oracle match_all lists (and the single-end oracle's states)"""
    og = ora.Genome(g.sym, g.frag_start)
    ix = ora.Index(og, seedl)
    p = ora.make_params(seedl=seedl, seedkmax=2, totalkmax=totalkmax, scores=scores, filter_level=filter_level, fileid=fileid)
    h1, o1, _ = ora.match_all(og, ix, p, b1.bases, b1.qual, b1.offsets)
    h2, o2, _ = ora.match_all(og, ix, p, b2.bases, b2.qual, b2.offsets)
    single = None
    if want_single:
        s1 = ora.unpack_record(ora.match_unique(og, ix, p, b1.bases, b1.qual, b1.offsets)[0])[0]
        s2 = ora.unpack_record(ora.match_unique(og, ix, p, b2.bases, b2.qual, b2.offsets)[0])[0]
        single = (s1, s2)
    return (fileid, h1, o1, h2, o2), single


def coverage(rec, single):
    """what a parametrisation must contain, computed from the checker's records"""
    st = rec["state"]
    uniq = st == UNIQUE
    return {"nomatch": int((st == NOMATCH).sum()), "unique": int(uniq.sum()), "nonunique": int((st == NONUNIQUE).sum()),
            "fwd_first": int((uniq & (rec["inverted1"] == 0)).sum()), "fwd_second": int((uniq & (rec["inverted1"] == 1)).sum()),
            "rescued": int((uniq & (single[0] == 4) & (single[1] == 4)).sum()) if single is not None else -1}
