"""Duplicate marking restated in numpy / pure Python -- TEST INFRASTRUCTURE ONLY (include/real_hip.h, "duplicates"): read
summaries, keys, dup[], statistics and the line `real -dedup 1` prints, from records and reads.  It never calls the code under
test and knows nothing of sort keys: a group is a dictionary entry.  Everything is an integer."""
from __future__ import annotations

import numpy as np

import pileup_checker as pk

SUM_DTYPE = np.dtype([("len", "<u4"), ("qsum", "<u4")])
UNIQUE = 1                          # REAL_HIP_PAIR_UNIQUE
STATS = ("reads", "placed", "groups", "duplicates")
DUP_FLAG = 1024


def summaries(qual, offsets, min_qual: int):
    """{len, qsum} of every read: qual the concatenated qualities (None: 30 per base), offsets the n + 1 starts"""
    off = np.asarray(offsets, dtype=np.int64)
    out = np.zeros(off.shape[0] - 1, dtype=SUM_DTYPE)
    out["len"] = off[1:] - off[:-1]
    for i in range(out.shape[0]):
        L = int(out["len"][i])
        if qual is None:
            out["qsum"][i] = 30 * L if 30 >= min_qual else 0
        else:
            q = np.asarray(qual[off[i]:off[i + 1]], dtype=np.int64)
            out["qsum"][i] = int(q[q >= min_qual].sum())
    return out


def summaries_of(b, min_qual: int):
    return summaries(b.qual, b.offsets, min_qual)


def keys_single(info, sums):
    """KEY (fileid, state, END5) of every placed read, None for the others"""
    info = np.asarray(info, dtype=np.uint64)
    out = []
    for i in range(info.shape[0]):
        r = int(info[i])
        state, fileid, pos = r >> 61, (r >> 35) & 63, r & ((1 << 35) - 1)
        if state not in (1, 2):
            out.append(None)
        else:
            out.append((fileid, state, pos if state == 1 else pos + int(sums["len"][i]) - 1))
    return out


def keys_pairs(pairs, s1, s2):
    """KEY (fileid, inverted1, START, END) of every placed fragment, None for the others"""
    out = []
    for i in range(pairs.shape[0]):
        r = pairs[i]
        if int(r["state"]) != UNIQUE:
            out.append(None)
            continue
        inv1 = 1 if int(r["inverted1"]) else 0
        f_pos, r_pos, len_r = (int(r["pos1"]), int(r["pos2"]), int(s2["len"][i])) if not inv1 else (int(r["pos2"]), int(r["pos1"]), int(s1["len"][i]))
        out.append((int(r["fileid"]), inv1, f_pos, r_pos + len_r - 1))
    return out


QSUM_TOP = (1 << 20) - 1             # "a qsum beyond 2^20 - 1 counts as 2^20 - 1" (per mate for pairs)


def clamped(qsum):
    return np.minimum(np.asarray(qsum, dtype=np.int64), QSUM_TOP)


def mark(keys, quality, quality2=None):
    """-> (dup, stats, groups): dup[i] = 1 iff record i has a key and is not its group's representative (largest quality, among
    equals the smallest index); groups: key -> the members' indices in ascending order.  quality: the qsum of every read,
    clamped here; quality2: for pairs the other mate's, clamped on its own and added"""
    quality = clamped(quality) if quality2 is None else clamped(quality) + clamped(quality2)
    groups = {}
    for i, k in enumerate(keys):
        if k is not None:
            groups.setdefault(k, []).append(i)
    dup = np.zeros(len(keys), dtype=np.uint8)
    for members in groups.values():
        rep = max(members, key=lambda i: (int(quality[i]), -i))
        for i in members:
            dup[i] = 0 if i == rep else 1
    placed = sum(len(m) for m in groups.values())
    return dup, {"reads": len(keys), "placed": placed, "groups": len(groups), "duplicates": placed - len(groups)}, groups


def mark_single(info, sums):
    return mark(keys_single(info, sums), sums["qsum"])


def mark_pairs(pairs, s1, s2):
    return mark(keys_pairs(pairs, s1, s2), s1["qsum"], s2["qsum"])


def representatives(groups, quality):
    return {k: max(m, key=lambda i: (int(quality[i]), -i)) for k, m in groups.items()}


def stderr_line(st, min_qual: int) -> str:
    return "duplicates: placed=%d groups=%d duplicates=%d rate=%.4f min_qual=%d" % (
        st["placed"], st["groups"], st["duplicates"], st["duplicates"] / st["placed"] if st["placed"] else 0.0, min_qual)


# ---- what the marks do to the outputs of `real` ---------------------------------------------------------------------------
def sam_with_marks(text: str, qnames) -> str:
    """sam_checker's text with 1024 added to the FLAG of every line whose QNAME is in qnames (a duplicate read is placed: it
    has one line; a duplicate fragment two)"""
    out = []
    for line in text.split("\n"):
        if line and not line.startswith("@"):
            f = line.split("\t")
            if f[0] in qnames:
                f[1] = str(int(f[1]) + DUP_FLAG)
                line = "\t".join(f)
        out.append(line)
    return "\n".join(out)


def masked_info(info, dup):
    """the records as the pileup sees them: a duplicate is NoMatch (word 0)"""
    return np.where(np.asarray(dup) != 0, np.uint64(0), np.asarray(info, dtype=np.uint64))


def masked_pairs(pairs, dup):
    out = pairs.copy()
    out["state"][np.asarray(dup) != 0] = 0
    return out


def pileup_single(sym, fileid, min_qual, b, info, dup):
    pu = pk.Pileup(sym, fileid, min_qual)
    pu.add(b, masked_info(info, dup))
    return pu


def pileup_pairs(sym, fileid, min_qual, b1, b2, pairs, dup):
    pu = pk.Pileup(sym, fileid, min_qual)
    pu.add_pairs(b1, b2, masked_pairs(pairs, dup))
    return pu
