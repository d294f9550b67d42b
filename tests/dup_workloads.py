"""The workloads the duplicate-marking tests share -- TEST INFRASTRUCTURE ONLY: the pileup's single-end batches with the oracle's
records (their hot spot is 300 copies of one read), and a paired workload derived from the insert-size one by appending copies of
every 50th fragment with fresh qualities and shortened 3' ends.  The checker is dup_checker.py."""
from __future__ import annotations

import functools

import numpy as np

import dup_checker as dk
import insert_workloads as iw
import pairs_checker as pc
import pairs_workloads as pairw
import pileup_workloads as pw

MIN_QUAL = 15                       # the default of -dedup_minq


@functools.lru_cache(maxsize=None)
def single_sums(which: str, min_qual: int = MIN_QUAL):
    return dk.summaries_of(getattr(pw.workload(), which), min_qual)


def single_expected(ora, which: str, scores: int = 1, min_qual: int = MIN_QUAL):
    """-> (the oracle's info, the checker's summaries, dup, stats, groups)"""
    info = pw.oracle_records(ora, which, scores)[0]
    sums = single_sums(which, min_qual)
    return (info, sums) + dk.mark_single(info, sums)


def groups_spanning_batches(groups, batch: int) -> int:
    return sum(1 for m in groups.values() if len(m) > 1 and len({i // batch for i in m}) > 1)


def assert_single_conditions(ora):
    """what the single-end workload must contain for the tests not to pass vacuously (figures of the main batch with scores on
    and min_qual 15, computed on the CPU)"""
    info, sums, dup, st, groups = single_expected(ora, "main")
    assert st == {"reads": 2014, "placed": 1926, "groups": 1622, "duplicates": 304}, st
    assert sorted(len(m) for m in groups.values())[-2:] == [145, 147]
    reps = dk.representatives(groups, sums["qsum"])
    assert sum(1 for k, m in groups.items() if len(m) > 1 and reps[k] != m[0]) == 9
    assert groups_spanning_batches(groups, 300) == 13
    top = [sorted((int(sums["qsum"][i]) for i in m), reverse=True) for m in groups.values() if len(m) > 1]
    assert sum(1 for q in top if q[0] == q[1]) == 0      # no group's best qsum is shared: the tie rule is covered by hand-made cases
    _, _, _, lst, _ = single_expected(ora, "long")
    assert lst["placed"] == 41 and lst["duplicates"] == 0


def _cut(b, i, head: int = 0, tail: int = 0):
    lo, hi = int(b.offsets[i]) + head, int(b.offsets[i + 1]) - tail
    return b.bases[lo:hi].copy(), hi - lo


@functools.lru_cache(maxsize=None)
def pair_workload():
    """(genome, mate batch 1, mate batch 2) with copies: from every 50th fragment starting at 3 (the j-th pick) (1, 2, 5)[j % 3]
    copies, each with fresh qualities uniform in 0..40 and each mate shortened at its 3' end by an independent 0..10 bases;
    where j % 4 == 0 one more copy whose mate 2 is shortened by 2 at its 5' END: another fragment, no duplicate"""
    from real_amd import synth
    g, b1, b2 = iw.workload("iid", True)
    rng = np.random.default_rng(5)
    extra = ([], [])
    ids = ([], [])
    for j, i in enumerate(range(3, b1.n_reads, 50)):
        shapes = [(int(rng.integers(0, 11)), int(rng.integers(0, 11)), 0) for _ in range((1, 2, 5)[j % 3])]
        if j % 4 == 0:
            shapes.append((0, 0, 2))
        for c, (t1, t2, h2) in enumerate(shapes):
            for m, (b, head, tail) in enumerate(((b1, 0, t1), (b2, h2, t2))):
                bases, L = _cut(b, i, head, tail)
                extra[m].append((bases, rng.integers(0, 41, size=L).astype(np.uint8)))
                stem, mate = b.ids[i].rsplit("/", 1)
                ids[m].append("%s_c%d/%s" % (stem, c, mate))
    out = []
    for m, b in enumerate((b1, b2)):
        lens = [x[0].shape[0] for x in extra[m]]
        add = synth.ReadBatch(bases=np.concatenate([x[0] for x in extra[m]]), qual=np.concatenate([x[1] for x in extra[m]]),
                              offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), ids=ids[m])
        out.append(synth.concat_batches([b, add]))
    return g, out[0], out[1]


_pairs = {}


def pair_lists(ora, scores: int = 1):
    if scores not in _pairs:
        g, b1, b2 = pair_workload()
        _pairs[scores] = pairw.oracle_pairs(ora, g, b1, b2, iw.SEEDL, iw.TOTALK, int(scores), iw.FILTER_LEVEL)[0]
    return _pairs[scores]


def pair_records(ora, scores: int = 1):
    g, b1, b2 = pair_workload()
    return pc.check_pairs([pair_lists(ora, scores)], pairw.lens_of(b1), pairw.lens_of(b2), iw.WINDOW[0], iw.WINDOW[1], int(scores),
                          ora.filter_mult(iw.FILTER_LEVEL, iw.TOTALK))


def pair_expected(ora, scores: int = 1, min_qual: int = MIN_QUAL):
    """-> (the checker's pair records, summaries of mate 1 and mate 2, dup, stats, groups)"""
    g, b1, b2 = pair_workload()
    rec = pair_records(ora, scores)
    s1, s2 = dk.summaries_of(b1, min_qual), dk.summaries_of(b2, min_qual)
    return (rec, s1, s2) + dk.mark_pairs(rec, s1, s2)


def assert_pair_conditions(ora):
    rec, s1, s2, dup, st, groups = pair_expected(ora)
    multi = [m for m in groups.values() if len(m) > 1]
    assert st["duplicates"] >= 100 and st["placed"] > 1800, st
    assert {int(rec["inverted1"][m[0]]) for m in multi} == {0, 1}
    assert sum(1 for m in multi if len({(int(s1["len"][i]), int(s2["len"][i])) for i in m}) > 1) >= 30
    assert max(len(m) for m in multi) >= 5


# ---- hand-made records: what the rules say where a workload would not show it ---------------------------------------------
def _info(state, pos, fileid=0):
    return (state << 61) | (fileid << 35) | pos


def _sums(rows):
    s = np.zeros(len(rows), dtype=dk.SUM_DTYPE)
    s["len"], s["qsum"] = [r[0] for r in rows], [r[1] for r in rows]
    return s


TOP_POS = (1 << 35) - 1             # the last position an info word can hold
MAX_QSUM = 16384 * 63


def hand_single():
    """-> (info, summaries, the marks the rules give, written down by hand)"""
    rows = [  # state, pos, fileid, len, qsum, dup
        (1, 1000, 0, 50, 100, 0),                 # 0 forward at 1000: the representative of {0, 5, 8} (tie with 5: the smallest index)
        (2, 951, 0, 50, 200, 1),                  # 1 reverse, END5 = 1000: not in 0's group (the strand differs); in 2's
        (2, 961, 0, 40, 300, 0),                  # 2 reverse of another length with pos + len - 1 = 1000: 1's group, the best
        (2, 951, 0, 60, 50, 0),                   # 3 reverse at 1's pos, another length: END5 = 1010, alone
        (1, 1000, 1, 50, 500, 0),                 # 4 another file id: alone
        (1, 1000, 0, 70, 100, 1),                 # 5 the tie with 0
        (0, 1000, 0, 50, 900, 0),                 # 6 NoMatch
        (4, 1000, 0, 50, 999, 0),                 # 7 NonUnique
        (1, 1000, 0, 50, 99, 1),                  # 8
        (1, 2000, 0, 33, 0, 1),                   # 9 qsum 0 and the largest qsum there is in one group
        (1, 2000, 0, 16384, MAX_QSUM, 0),         # 10
        (2, TOP_POS, 0, 16384, 5, 1),             # 11 END5 = 2^35 + 16382: 36 bits
        (2, TOP_POS + 16384 - 20000, 0, 20000, 6, 0),   # 12 the same END5 through another length (the marking takes len as it is)
        (2, TOP_POS + 16384 - 20000, 0, 16384, 7, 0),   # 13 12's pos with 11's length: alone
        (3, 2000, 0, 33, 5, 0),                   # 14 state 3: not placed
    ]
    info = np.array([_info(r[0], r[1], r[2]) for r in rows], dtype=np.uint64)
    return info, _sums([(r[3], r[4]) for r in rows]), np.array([r[5] for r in rows], dtype=np.uint8)


def hand_pairs():
    """-> (pair records, summaries of mate 1 and of mate 2, the marks written down by hand)"""
    top = (1 << 32) - 1
    rows = [  # state, fileid, inverted1, pos1, pos2, (len1, q1), (len2, q2), dup
        (1, 0, 0, 100, 300, (80, 10), (50, 10), 1),          # 0 START 100, END 349
        (1, 0, 1, 300, 100, (50, 25), (80, 25), 0),          # 1 the same START and END with mate 2 forward: inverted1 differs, alone
        (1, 0, 0, 100, 310, (70, 10), (40, 20), 0),          # 2 END 349 through another len_r: 0's group, the best (tie with 10)
        (1, 0, 0, 100, 300, (80, 40), (60, 40), 0),          # 3 equal START, END 359: alone
        (1, 1, 0, 100, 300, (80, 40), (50, 40), 0),          # 4 another file id: alone
        (1, 0, 0, 5, top, (50, 3), (16384, 4), 0),           # 5 END = 2^32 + 16382: 33 bits
        (1, 0, 0, 5, top + 16384 - 20000, (50, 1), (20000, 2), 1),   # 6 the same END through another length
        (1, 0, 0, 5, 16333, (50, 50), (50, 50), 0),          # 7 END = 16382: 5's without bit 32, alone
        (0, 0, 0, 100, 300, (80, 60), (50, 60), 0),          # 8 NoMatch
        (2, 0, 0, 100, 300, (80, 60), (50, 60), 0),          # 9 NonUnique
        (1, 0, 0, 100, 310, (60, 25), (40, 5), 1),           # 10 the quality tie with 2: 30 = 30, the smaller index stays
    ]
    pairs = np.zeros(len(rows), dtype=pc.REC_DTYPE)
    for k, col in (("state", 0), ("fileid", 1), ("inverted1", 2), ("pos1", 3), ("pos2", 4)):
        pairs[k] = [r[col] for r in rows]
    return pairs, _sums([r[5] for r in rows]), _sums([r[6] for r in rows]), np.array([r[7] for r in rows], dtype=np.uint8)


def synthetic_records(n: int = 300_000, sites: int = 50_000, seed: int = 9):
    """records alone, no reads: n placed or unplaced info words over `sites` positions, both strands, two file ids"""
    rng = np.random.default_rng(seed)
    site = rng.integers(0, sites, size=n).astype(np.uint64) * np.uint64(7) + np.uint64(100)
    state = rng.choice(np.array([0, 1, 1, 1, 2, 2, 2, 4], dtype=np.uint64), size=n)
    fileid = (rng.random(n) < 0.1).astype(np.uint64)
    sums = np.zeros(n, dtype=dk.SUM_DTYPE)
    sums["len"] = rng.integers(30, 40, size=n)
    sums["qsum"] = rng.integers(0, 64, size=n)        # (a narrow range: many ties)
    return (state << np.uint64(61)) | (fileid << np.uint64(35)) | site, sums
