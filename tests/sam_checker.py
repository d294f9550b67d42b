"""The mismatch lists and `real -sam` restated in numpy -- TEST INFRASTRUCTURE ONLY (include/real_hip.h, "mismatch lists";
DESIGN.md 7c).  Fed the ORACLE's records (and the pair / single checkers' over the oracle's lists) and never the code under
test: the final placement of every read, its list, the statistics with `disagree`, NM / MD, and the whole SAM text
(header, flags, order of the lines).  Everything is an integer or a string."""
from __future__ import annotations

import types

import numpy as np

UNIQUE, NOMATCH = 1, 0              # REAL_HIP_PAIR_UNIQUE / _NOMATCH
MM_DTYPE = np.dtype([("off", "<u2"), ("ref", "u1"), ("base", "u1")])
COUNTERS = ("reads", "placed", "other_file", "invalid", "bases", "mismatches", "on_n", "disagree")


# ---- the final placement of every list ----------------------------------------------------------------------------
def _fin(n):
    return types.SimpleNamespace(placed=np.zeros(n, bool), inv=np.zeros(n, bool), fileid=np.zeros(n, np.int64), frag=np.zeros(n, np.int64),
                                 pos=np.zeros(n, np.int64), k=np.zeros(n, np.int64), score=np.zeros(n, np.float32), paired=np.zeros(n, bool))


def final_single(info, score=None):
    """single-end: a record of state 1 or 2 places its read, reverse iff the state is 2"""
    info = np.asarray(info, dtype=np.uint64)
    f = _fin(info.shape[0])
    st = (info >> np.uint64(61)).astype(np.int64)
    f.placed[:] = (st == 1) | (st == 2)
    f.inv[:] = st == 2
    f.frag[:] = ((info >> np.uint64(45)) & np.uint64(0xffff)).astype(np.int64)
    f.k[:] = ((info >> np.uint64(41)) & np.uint64(15)).astype(np.int64)
    f.fileid[:] = ((info >> np.uint64(35)) & np.uint64(63)).astype(np.int64)
    f.pos[:] = (info & np.uint64((1 << 35) - 1)).astype(np.int64)
    if score is not None:
        f.score[:] = score
    return f


def final_pairs(pairs, s1=None, s2=None):
    """paired-end, list 2i = mate 1, 2i + 1 = mate 2 of fragment i: the pair record if it is Unique; else the mate's single
    record if it is Unique -- only when singles are given and the pair record is NoMatch"""
    n = int(pairs.shape[0])
    f = _fin(2 * n)
    for i in range(n):
        P = pairs[i]
        if P["state"] == UNIQUE:
            for m in (0, 1):
                j = 2 * i + m
                f.placed[j], f.paired[j] = True, True
                f.inv[j] = bool(P["inverted1"]) != bool(m)
                f.fileid[j], f.frag[j] = int(P["fileid"]), int(P["frag"])
                f.pos[j], f.k[j], f.score[j] = int(P["pos2" if m else "pos1"]), int(P["k2" if m else "k1"]), P["score2" if m else "score1"]
        elif P["state"] == NOMATCH and s1 is not None:
            for m, S in ((0, s1[i]), (1, s2[i])):
                tag = int(S["tag"])
                if (tag >> 5) & 3 != UNIQUE:
                    continue
                j = 2 * i + m
                f.placed[j] = True
                f.inv[j] = bool((tag >> 4) & 1)
                f.fileid[j], f.frag[j], f.pos[j], f.k[j], f.score[j] = int(S["fileid"]), int(S["frag"]), int(S["pos"]), tag & 15, S["score"]
    return f


def single_reads(b):
    """list j -> the bases of read j of a batch"""
    return lambda j: b.bases[int(b.offsets[j]):int(b.offsets[j + 1])]


def pair_reads(b1, b2):
    return lambda j: (b2 if j & 1 else b1).bases[int((b2 if j & 1 else b1).offsets[j >> 1]):int((b2 if j & 1 else b1).offsets[(j >> 1) + 1])]


# ---- the lists ------------------------------------------------------------------------------------------------------------
def placement_list(sym, read, p: int, inverted: bool):
    """the list of one placement: every offset on an N of the text (ref 4), elsewhere every offset where the oriented base differs"""
    read = np.asarray(read, dtype=np.int64)
    o = 3 - read[::-1] if inverted else read
    t = np.asarray(sym[p:p + o.shape[0]], dtype=np.int64)
    at = np.nonzero((t > 3) | (o != t))[0]
    out = np.zeros(at.shape[0], dtype=MM_DTYPE)
    out["off"], out["ref"], out["base"] = at, np.minimum(t[at], 4), o[at]
    return out


def mismatch_lists(sym, fileid: int, fin, reads):
    """-> (lists concatenated, offsets of len(lists) + 1, statistics) over the text `sym` of file `fileid`"""
    n_lists = int(fin.placed.shape[0])
    st = {k: 0 for k in COUNTERS}
    st["reads"] = n_lists
    parts, off = [], np.zeros(n_lists + 1, dtype=np.uint64)
    n = int(np.asarray(sym).shape[0])
    for j in range(n_lists):
        off[j + 1] = off[j]
        if not fin.placed[j]:
            continue
        if int(fin.fileid[j]) != fileid:
            st["other_file"] += 1
            continue
        r = reads(j)
        if int(fin.pos[j]) + int(r.shape[0]) > n:
            st["invalid"] += 1
            continue
        L = placement_list(sym, r, int(fin.pos[j]), bool(fin.inv[j]))
        st["placed"] += 1
        st["bases"] += int(r.shape[0])
        st["mismatches"] += int(L.shape[0])
        st["on_n"] += int((L["ref"] == 4).sum())
        st["disagree"] += int(L.shape[0] != int(fin.k[j]))
        parts.append(L)
        off[j + 1] += L.shape[0]
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=MM_DTYPE)), off, st


def md_of(L, length: int) -> str:
    """MD:Z: from a list: the decimal run of matches, then the letter of the text there, alternating; a number at either end"""
    out, last = [], 0
    for e in L:
        out.append("%d%s" % (int(e["off"]) - last, "ACGTN"[int(e["ref"])]))
        last = int(e["off"]) + 1
    return "".join(out) + "%d" % (length - last)


def reference_from_md(seq: str, md: str) -> str:
    """the text under a placed line, rebuilt from SEQ and MD alone"""
    ref, i, num = [], 0, ""
    for c in md + "$":
        if c.isdigit():
            num += c
            continue
        ref.append(seq[i:i + int(num)])
        i += int(num)
        num = ""
        if c != "$":
            ref.append(c)
            i += 1
    assert i == len(seq), (i, len(seq), md)
    return "".join(ref)


# ---- the SAM text ---------------------------------------------------------------------------------------------------------
def frag_name(name: str) -> str:
    return name.split()[0]


def qname(read_id: str, paired: bool) -> str:
    q = read_id.replace("\t", " ").split(" ")[0]
    return q[:-2] if paired and (q.endswith("/1") or q.endswith("/2")) else q


def header(genomes) -> str:
    sq = "".join("@SQ\tSN:%s\tLN:%d\n" % (frag_name(g.frag_names[f]), int(g.frag_start[f + 1]) - int(g.frag_start[f]))
                 for g in genomes for f in range(len(g.frag_names)))
    return "@HD\tVN:1.6\tSO:unknown\n" + sq + "@PG\tID:real\n"


def _seq_qual(b, i, inverted, fastq):
    lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
    bases = b.bases[lo:hi]
    seq = "".join("ACGTN"[min(int(c), 4)] for c in ((3 - bases[::-1]) if inverted else bases))
    if not fastq:
        return seq, "*"
    q = b.qual[lo:hi][::-1] if inverted else b.qual[lo:hi]
    return seq, "".join(chr(int(v) + 33) for v in q)


def _fmt_score(x) -> str:
    return "%g" % float(np.float32(x))


def _tags(L, length, score, scores):
    return ["NM:i:%d" % L.shape[0], "MD:Z:" + md_of(L, length)] + (["ZS:f:" + _fmt_score(score)] if scores else [])


def _where(genomes, fin, j):
    g = genomes[int(fin.fileid[j])]
    return frag_name(g.frag_names[int(fin.frag[j])]), int(fin.pos[j]) - int(g.frag_start[int(fin.frag[j])]) + 1


def sam_single(genomes, b, info, score, scores: bool, fastq: bool = True):
    """-> (the whole -sam file of a single-end run, the per-file statistics): per genome file the reads placed in it in read
    order; the reads without a placement in the pass of the last file, at their place"""
    fin = final_single(info, score if scores else None)
    out, stats = [header(genomes)], []
    for fi, g in enumerate(genomes):
        lists, off, st = mismatch_lists(g.sym, fi, fin, single_reads(b))
        stats.append(st)
        for i in range(b.n_reads):
            q = qname(b.ids[i], False)
            L = int(b.offsets[i + 1]) - int(b.offsets[i])
            if fin.placed[i] and int(fin.fileid[i]) == fi:
                seq, qual = _seq_qual(b, i, bool(fin.inv[i]), fastq)
                name, pos = _where(genomes, fin, i)
                out.append("\t".join([q, "16" if fin.inv[i] else "0", name, str(pos), "255", "%dM" % L, "*", "0", "0", seq, qual] +
                                     _tags(lists[int(off[i]):int(off[i + 1])], L, fin.score[i], scores)) + "\n")
            elif not fin.placed[i] and fi == len(genomes) - 1:
                seq, qual = _seq_qual(b, i, False, fastq)
                out.append("\t".join([q, "4", "*", "0", "0", "*", "*", "0", "0", seq, qual]) + "\n")
    return "".join(out), stats


def sam_pairs(genomes, b1, b2, pairs, s1, s2, scores: bool, fastq=(True, True)):
    """-> (the whole -sam file of a -p2 run, the per-file statistics).  In the pass of file fi a mate is written if it is placed
    in fi, or if it is unplaced and its mate is placed in fi (beside it, mate 1 first); fragments with nothing placed in the
    pass of the last file"""
    fin = final_pairs(pairs, s1, s2)
    bs = (b1, b2)
    out, stats = [header(genomes)], []
    for fi, g in enumerate(genomes):
        lists, off, st = mismatch_lists(g.sym, fi, fin, pair_reads(b1, b2))
        stats.append(st)
        for i in range(b1.n_reads):
            for m in (0, 1):
                j, o = 2 * i + m, 2 * i + 1 - m
                b = bs[m]
                here = fin.placed[j] and int(fin.fileid[j]) == fi
                beside = not fin.placed[j] and fin.placed[o] and int(fin.fileid[o]) == fi
                nothing = not fin.placed[j] and not fin.placed[o] and fi == len(genomes) - 1
                if not (here or beside or nothing):
                    continue
                L = int(b.offsets[i + 1]) - int(b.offsets[i])
                flag = 1 | (64 if m == 0 else 128)
                flag |= 2 if (fin.placed[j] and fin.paired[j]) else 0
                flag |= 0 if fin.placed[j] else 4
                flag |= 0 if fin.placed[o] else 8
                flag |= 16 if (fin.placed[j] and fin.inv[j]) else 0
                flag |= 32 if (fin.placed[o] and fin.inv[o]) else 0
                q = qname(b.ids[i], True)
                if fin.placed[j]:
                    seq, qual = _seq_qual(b, i, bool(fin.inv[j]), fastq[m])
                    name, pos = _where(genomes, fin, j)
                    rnext, pnext, tlen = "=", pos, 0
                    if fin.placed[o]:
                        oname, opos = _where(genomes, fin, o)
                        same = int(fin.fileid[o]) == int(fin.fileid[j]) and int(fin.frag[o]) == int(fin.frag[j])
                        rnext, pnext = ("=" if same else oname), opos
                        if fin.paired[j]:
                            fw, rv = (o, j) if fin.inv[j] else (j, o)
                            lr = int(bs[rv & 1].offsets[i + 1]) - int(bs[rv & 1].offsets[i])
                            outer = int(fin.pos[rv]) + lr - int(fin.pos[fw])
                            tlen = -outer if fin.inv[j] else outer
                    out.append("\t".join([q, str(flag), name, str(pos), "255", "%dM" % L, rnext, str(pnext), str(tlen), seq, qual] +
                                         _tags(lists[int(off[j]):int(off[j + 1])], L, fin.score[j], scores)) + "\n")
                else:
                    seq, qual = _seq_qual(b, i, False, fastq[m])
                    if fin.placed[o]:
                        oname, opos = _where(genomes, fin, o)
                        where = [oname, str(opos), "0", "*", "=", str(opos), "0"]
                    else:
                        where = ["*", "0", "0", "*", "*", "0", "0"]
                    out.append("\t".join([q, str(flag)] + where + [seq, qual]) + "\n")
    return "".join(out), stats


def stderr_line(st, name: str) -> str:
    return "sam: file=%s placements=%d mismatches=%d on_n=%d disagree=%d" % (name, st["placed"], st["mismatches"], st["on_n"], st["disagree"])
