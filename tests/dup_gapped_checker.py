"""The joint duplicate marking over info words and gap records restated in numpy / pure Python -- TEST INFRASTRUCTURE ONLY
(include/real_hip.h, "duplicates", SINGLE-END WITH GAPPED PLACEMENTS).  Two formulations that share nothing but
the decoding of the records: a dictionary of groups (dup_checker.mark) and a sort by (key, -qsum, index).  Neither calls the code
under test.  Everything is an integer."""
from __future__ import annotations

import numpy as np

import dup_checker as dk
import gap_checker as gc

E5_MOD = 1 << 36                     # "END5 is taken modulo 2^36"
UNGAPPED, GAPPED = 1, 2              # what places a read: its info word, its gap record


def gap_tag(state, inverted, target=0):
    """the tag byte of a gap record: bit 0 the target mate, bit 4 inverted, bits 5-6 the state"""
    return (target & 1) | ((1 if inverted else 0) << 4) | ((state & 3) << 5)


def placements(info, gaps, sums):
    """-> (kind, fileid, reverse, end5) per read as int64 arrays: kind 0 = not placed, UNGAPPED = by its info word (it wins),
    GAPPED = by its Unique gap record.  END5 in 64 bits, then modulo 2^36; the file id modulo 64"""
    info = np.asarray(info, dtype=np.uint64)
    n = info.shape[0]
    kind, fileid, rev, end5 = (np.zeros(n, dtype=np.int64) for _ in range(4))
    for i in range(n):
        w = int(info[i])
        state, L = w >> 61, int(sums["len"][i])
        if state in (1, 2):
            pos = w & ((1 << 35) - 1)
            kind[i], fileid[i], rev[i] = UNGAPPED, (w >> 35) & 63, state == 2
            end5[i] = (pos + L - 1 if state == 2 else pos) % E5_MOD
            continue
        g = gaps[i]
        tag = int(g["tag"])
        if (tag >> 5) & 3 != gc.UNIQUE:
            continue
        inv = (tag >> 4) & 1
        kind[i], fileid[i], rev[i] = GAPPED, int(g["fileid"]) % 64, inv
        end5[i] = (int(g["pos"]) + L + int(g["gap"]) - 1 if inv else int(g["pos"])) % E5_MOD
    return kind, fileid, rev, end5


def keys(info, gaps, sums):
    """KEY (fileid, reverse, END5) of every placed read, None for the others: one key space for both kinds"""
    kind, fileid, rev, end5 = placements(info, gaps, sums)
    return [None if not kind[i] else (int(fileid[i]), int(rev[i]), int(end5[i])) for i in range(kind.shape[0])]


def mark_groups(info, gaps, sums):
    """formulation 1, a dictionary of groups -> (dup, stats, groups) as dup_checker.mark"""
    return dk.mark(keys(info, gaps, sums), sums["qsum"])


def mark_sorted(info, gaps, sums):
    """formulation 2, one sort: the placed reads by (key, -clamped qsum, index); a read whose predecessor has its key is a
    duplicate -> (dup, stats)"""
    kind, fileid, rev, end5 = placements(info, gaps, sums)
    n = kind.shape[0]
    q = dk.clamped(sums["qsum"])
    idx = np.nonzero(kind)[0]
    word = (fileid[idx] << 37) | (rev[idx] << 36) | end5[idx]
    order = np.lexsort((idx, -q[idx], word))      # (the last key is the primary one)
    sw = word[order]
    first = np.ones(order.shape[0], dtype=bool)
    first[1:] = sw[1:] != sw[:-1]
    dup = np.zeros(n, dtype=np.uint8)
    dup[idx[order[~first]]] = 1
    placed, groups = int(idx.shape[0]), int(first.sum())
    return dup, {"reads": n, "placed": placed, "groups": groups, "duplicates": placed - groups}


def group_kinds(info, gaps, sums):
    """-> {key: (ungapped members, gapped members)} of the groups with more than one read"""
    kind = placements(info, gaps, sums)[0]
    out = {}
    for k, members in mark_groups(info, gaps, sums)[2].items():
        if len(members) > 1:
            out[k] = ([i for i in members if kind[i] == UNGAPPED], [i for i in members if kind[i] == GAPPED])
    return out


def gapped_line(info, gaps, sums, dup=None) -> str:
    """the second line `real -dedup 1` prints in a single-end run with gapped consumers: the Unique gap records (match_gapped
    writes one only for a read its info word places nowhere), and those of them that are marked"""
    unique = ((np.asarray(gaps["tag"], dtype=np.int64) >> 5) & 3) == gc.UNIQUE
    if dup is None:
        dup = mark_groups(info, gaps, sums)[0]
    return "duplicates gapped: placements=%d duplicates=%d" % (int(unique.sum()), int((unique & (np.asarray(dup) != 0)).sum()))


def masked_gaps(gaps, dup):
    """the gap records as the pileup and the calls see them: a duplicate is the NoMatch record"""
    out = np.array(gaps, dtype=gc.REC_DTYPE, copy=True)
    out[np.asarray(dup) != 0] = gc.empty_records(1)[0]
    return out
