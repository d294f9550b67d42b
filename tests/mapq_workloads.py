"""What the mapping quality tests share -- TEST INFRASTRUCTURE ONLY: over the parametrisations of singles_workloads (the same
genomes, reads and oracle lists), the checker's accumulators and qualities, computed once per parametrisation and left
unchanged, and the coverage every parametrisation must have."""
from __future__ import annotations

import numpy as np

import mapq_checker as mq
import pairs_workloads as pw
import singles_workloads as sw

CASES, KINDS = sw.CASES, sw.KINDS
# From the CPU oracle's lists, over the eight parametrisations: reads (of both mates) with two or more candidates: 462 at
# least.  Distinct MAPQ values among the placed mates: the iid genomes give 60 alone (a Unique placement there has no other
# candidate within the window's 15.5 bits) -- the repeat families are what gives more: 3 at least (28, 43, 60 with scores; 17,
# 27, 36, 60 without) where mismatches are allowed, and 60 alone with -e 0 (all candidates of a read are then equal).  Every
# families case has lists and products beyond a lane's budget (298 / 110 at least), the iid cases have none.  The tests ask
# for these floors.
NEED = {"two_or_more": 462}


def need_distinct(kind, case):
    return 3 if kind == "families" and case[1] > 0 else 1


_cache = {}


def workload(ora, kind, case):
    """singles_workloads.workload's dict, and: accp / acc1 / acc2 = the checker's accumulators (lists of dicts), mapq = the 2n
    bytes of the finish over the checker's records, placements / unlisted, cov"""
    key = (kind, case)
    if key not in _cache:
        w = dict(sw.workload(ora, kind, case))
        scores, w["case"] = case[0], case
        _, h1, o1, h2, o2 = w["f"]
        n = len(w["l1"])
        w["accp"] = mq.check_pair_hits([(h1, o1, h2, o2)], w["l1"], w["l2"], pw.MIN_INS, pw.MAX_INS, scores)
        w["acc1"], w["acc2"] = mq.check_hits([(h1, o1)], n, scores), mq.check_hits([(h2, o2)], n, scores)
        w["mapq"], w["placements"], w["unlisted"] = mq.finish_pairs(w["pairs"], w["s1"], w["s2"], w["accp"], w["acc1"], w["acc2"], scores)
        w["mapq_pairs_only"] = mq.finish_pairs(w["pairs"], None, None, w["accp"], None, None, scores)[0]
        w["products"] = int(((o1[1:] - o1[:-1]) * (o2[1:] - o2[:-1])).sum())
        w["products_beyond_32"] = int((((o1[1:] - o1[:-1]) * (o2[1:] - o2[:-1])) > 32).sum())
        w["cov"] = {"two_or_more": int(((o1[1:] - o1[:-1]) >= 2).sum() + ((o2[1:] - o2[:-1]) >= 2).sum()),
                    "distinct": len(set(int(q) for q in w["mapq"]) - {mq.NONE})}
        _cache[key] = w
    return _cache[key]


def assert_coverage(w, kind):
    for name, floor in NEED.items():
        assert w["cov"][name] >= floor, (name, w["cov"])
    assert w["cov"]["distinct"] >= need_distinct(kind, w["case"]), w["cov"]
    assert w["unlisted"] == 0, "seed hits alone: every placement is one of its accumulator's candidates"
    if kind == "families":
        assert w["longer_than_32"] > 0 and w["products_beyond_32"] > 0, "a 60-copy family gives lists beyond a lane's budget"


# ---- a genome with diverged copies: placements that are Unique and still not sure -----------------------------------------
NC_SIZE, NC_SEG, NC_SEGS, NC_SEEDL, NC_TOTALK, NC_INS = 200_000, 420, 40, 32, 3, (150, 420)


def near_copy_workload():
    """(genome, single-end reads, mate batch 1, mate batch 2): an iid genome in which NC_SEGS stretches of NC_SEG bases exist a
    second time with a substitution every 100 bases (the first half of them) or every 50 (the second half).  A 100-base read
    from such a stretch has its copy as a candidate one or two mismatches below: Unique where the mismatch's quality puts the
    copy beyond eps, and then with a mapping quality below 60 -- what -pileup_minmapq is for.  The fragments are 300 bases,
    mate 1 forward at the start and mate 2 reverse at the end; a third of the reads and fragments lie elsewhere."""
    if "nc" not in _cache:
        from pileup_workloads import _sample
        from real_amd import synth
        g = synth.random_genome(NC_SIZE, seed=61)
        rng = np.random.default_rng(62)
        src = [5_000 + 2_000 * k for k in range(NC_SEGS)]
        for k, s in enumerate(src):
            d = 100_000 + 2_000 * k
            g.sym[d:d + NC_SEG] = g.sym[s:s + NC_SEG]
            for x in range(25, NC_SEG, 100 if k < NC_SEGS // 2 else 50):
                g.sym[d + x] = (g.sym[d + x] + 1 + k % 3) & 3
        starts = [s + int(rng.integers(0, NC_SEG - 300)) for s in src for _ in range(12)] + [int(v) for v in rng.integers(185_000, 199_000, size=240)]
        single = _sample(rng, g.sym, [(p + (100 if i % 3 == 0 else 0), 100, bool(i & 1)) for i, p in enumerate(starts)], 0.01, "n")
        fwd1 = [bool(i % 4 < 2) for i in range(len(starts))]        # mate 1 is the forward mate in half of the fragments
        b1 = _sample(rng, g.sym, [(p if f else p + 200, 100, not f) for p, f in zip(starts, fwd1)], 0.01, "f")
        b2 = _sample(rng, g.sym, [(p + 200 if f else p, 100, f) for p, f in zip(starts, fwd1)], 0.01, "f")
        _cache["nc"] = (g, single, b1, b2)
    return _cache["nc"]
