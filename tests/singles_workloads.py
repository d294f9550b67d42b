"""What the tests of the single placements of a mate share -- TEST INFRASTRUCTURE ONLY: the parametrisations of the
whole-path tests over pairs_workloads.pair_workload, and their oracle lists and checker records, computed once per
parametrisation and left unchanged."""
from __future__ import annotations

import pairs_checker as pc
import pairs_workloads as pw
import singles_checker as sc

# scores, totalkmax, filter_level, seedl, ragged, (patl1, patl2), table_kind, prefix_bits
CASES = [(1, 3, 2, 32, False, (100, 100), 0, 0),
         (0, 3, 2, 16, False, (100, 80), 3, 13),
         (1, 3, 2, 16, True, (100, 100), 3, 13),
         (0, 0, 2, 32, True, (100, 80), 0, 0)]
KINDS = ["iid", "families"]
# the smallest counts over the eight parametrisations, from the CPU oracle's lists, are 8 / 79 / 15 / 2 (and 298 lists
# longer than a lane's budget in a families case); the tests ask for these floors
NEED = {"both_unique": 5, "one_unique": 5, "a_nonunique": 5, "neither": 1}

_cache = {}


def workload(ora, kind, case):
    """dict: g, b1, b2, f = (fileid, h1, o1, h2, o2), pairs / s1 / s2 = the checkers' records, classes, longer_than_32"""
    key = (kind, case)
    if key not in _cache:
        scores, tk, fl, seedl, ragged, patl, _, _ = case
        g, b1, b2 = pw.pair_workload(kind, ragged, patl)
        f, _ = pw.oracle_pairs(ora, g, b1, b2, seedl, tk, scores, fl)
        fm = ora.filter_mult(fl, tk)
        l1, l2 = pw.lens_of(b1), pw.lens_of(b2)
        pairs = pc.check_pairs([f], l1, l2, pw.MIN_INS, pw.MAX_INS, scores, fm)
        s1 = sc.check_singles([(0, f[1], f[2])], l1, scores, fm)
        s2 = sc.check_singles([(0, f[3], f[4])], l2, scores, fm)
        longer = int(((f[2][1:] - f[2][:-1]) > 32).sum() + ((f[4][1:] - f[4][:-1]) > 32).sum())
        _cache[key] = {"g": g, "b1": b1, "b2": b2, "f": f, "fm": fm, "l1": l1, "l2": l2, "pairs": pairs, "s1": s1, "s2": s2,
                       "classes": sc.classes(pairs["state"], s1, s2), "longer_than_32": longer,
                       "hits": int(f[2][-1]) + int(f[4][-1])}
    return _cache[key]


def assert_coverage(w, kind):
    for name, floor in NEED.items():
        assert w["classes"][name] >= floor, (name, w["classes"])
    if kind == "families":
        assert w["longer_than_32"] > 0, "a 60-copy family gives lists beyond a lane's budget"
