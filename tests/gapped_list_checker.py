"""The checker of the gapped mismatch lists and of `real -sam_gapped 1` -- TEST INFRASTRUCTURE ONLY.

A numpy statement of include/real_hip.h, "gapped mismatch lists", over the reads, the gap records and the text.  It never calls
the code under test and imports nothing of the product.  Two formulations of the list of one placement:
  list_by_pairs      the aligned (read offset, text position) pairs are built explicitly (gap_checker.aligned_pairs) and compared
                     one by one; the deleted range is added;
  list_by_diagonals  the difference vectors of the two diagonals (read against text at p, read against text at p + g), cut at
                     the split, in numpy.
Then NM / MD from a list, the text span rebuilt from SEQ, CIGAR and MD alone, and the SAM lines of a fragment with a rescued
mate on sam_checker.sam_pairs' pieces.  Everything is an integer or a string.
"""
from __future__ import annotations

import re

import numpy as np

import gap_checker as gc
import sam_checker as sk

MM_DTYPE = sk.MM_DTYPE
DELETED = 4
COUNTERS = ("fragments", "placed", "other_file", "invalid", "aligned_bases", "mismatches", "deleted", "inserted", "on_n", "disagree")


def fits(rec, l: int, n: int) -> bool:
    """the geometry of a Unique record of the resident file: does it describe a placement of a read of l bases inside n"""
    g, j, p = int(rec["gap"]), int(rec["split"]), int(rec["pos"])
    d = max(-g, 0)
    if abs(g) > gc.GAP_MAX or l > gc.MAX_PATL:
        return False
    if g != 0 and not (1 <= j and j + d <= l - 1):
        return False
    if g == 0 and j != 0:
        return False
    return p + l + g <= n


def _entries(rows):
    out = np.zeros(len(rows), dtype=MM_DTYPE)
    for k, (off, ref, base) in enumerate(rows):
        out[k] = (off, ref, base)
    return out


def list_by_pairs(sym, r, p: int, g: int, j: int):
    """r: the ORIENTED read.  One entry per deleted text position and per aligned pair on an N or with differing bases"""
    l = int(r.shape[0])
    rows = []
    for i, x in gc.aligned_pairs(l, p, g, j):
        t = int(sym[x])
        if t > 3 or t != int(r[i]):
            rows.append((x - p, min(t, 4), int(r[i])))
    if g > 0:
        rows += [(t, min(int(sym[p + t]), 4), DELETED) for t in range(j, j + g)]
    return _entries(sorted(rows))


def list_by_diagonals(sym, r, p: int, g: int, j: int):
    """the same list from the two diagonals: text offset t meets read offset t on the first, read offset t - g on the second"""
    l = int(r.shape[0])
    span = l + g
    t = np.arange(span, dtype=np.int64)
    txt = np.minimum(np.asarray(sym[p:p + span], dtype=np.int64), 4)
    rr = np.asarray(r, dtype=np.int64)
    first = np.where(t < l, rr[np.clip(t, 0, l - 1)], -1)                  # the read on the diagonal of p
    second = np.where((t - g >= 0) & (t - g < l), rr[np.clip(t - g, 0, l - 1)], -1)   # and on the diagonal of p + g
    if g == 0:
        on_first, on_second = np.ones(span, bool), np.zeros(span, bool)
    else:
        on_first, on_second = t < j, t >= j + max(g, 0)
    base = np.where(on_first, first, np.where(on_second, second, DELETED))
    listed = ~(on_first | on_second) | (txt > 3) | (base != txt)
    at = np.nonzero(listed)[0]
    out = np.zeros(at.shape[0], dtype=MM_DTYPE)
    out["off"], out["ref"], out["base"] = at, txt[at], base[at]
    return out


def target_read(b1, b2, rec, i):
    b = (b1, b2)[int(gc.target_of(rec["tag"]))]
    return b.bases[int(b.offsets[i]):int(b.offsets[i + 1])]


def gapped_lists(sym, fileid: int, b1, b2, gaps, one_list=list_by_pairs):
    """-> (lists concatenated, offsets of n + 1, counters) over the text `sym` of file `fileid`"""
    n = int(gaps.shape[0])
    sym = np.asarray(sym)
    ctr = dict.fromkeys(COUNTERS, 0)
    ctr["fragments"] = n
    parts, off = [], np.zeros(n + 1, dtype=np.uint64)
    for i in range(n):
        off[i + 1] = off[i]
        rec = gaps[i]
        if int(gc.state_of(rec["tag"])) != gc.UNIQUE:
            continue
        if int(rec["fileid"]) != fileid:
            ctr["other_file"] += 1
            continue
        read = target_read(b1, b2, rec, i)
        l = int(read.shape[0])
        if not fits(rec, l, int(sym.shape[0])):
            ctr["invalid"] += 1
            continue
        g, j = int(rec["gap"]), int(rec["split"])
        L = one_list(sym, gc.oriented(read, bool(gc.inverted_of(rec["tag"]))), int(rec["pos"]), g, j)
        aligned = int((L["base"] != DELETED).sum())
        ctr["placed"] += 1
        ctr["aligned_bases"] += l - max(-g, 0)
        ctr["mismatches"] += aligned
        ctr["deleted"] += max(g, 0)
        ctr["inserted"] += max(-g, 0)
        ctr["on_n"] += int((L["ref"] == 4).sum())
        ctr["disagree"] += int(aligned != int(rec["k"]))
        assert int(L.shape[0]) == aligned + max(g, 0)
        parts.append(L)
        off[i + 1] += L.shape[0]
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=MM_DTYPE)), off, ctr


# ---- NM / MD / the reference back from a line ------------------------------------------------------------------------------
def nm_of(L, g: int) -> int:
    return int(L.shape[0]) + max(-g, 0)


def md_of(L, span: int) -> str:
    """MD:Z: [0-9]+(([A-Z]|\\^[A-Z]+)[0-9]+)*: a number between any two items, a run of deleted entries as ^ and its letters"""
    out, last, in_del = [], 0, False
    for e in L:
        off, deleted = int(e["off"]), int(e["base"]) == DELETED
        if not (deleted and in_del and off == last):
            out.append("%d" % (off - last))
            if deleted:
                out.append("^")
        out.append("ACGTN"[int(e["ref"])])
        last, in_del = off + 1, deleted
    return "".join(out) + "%d" % (span - last)


MD_RE = re.compile(r"^[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*$")


def reference_from_cigar_md(seq: str, cigar: str, md: str) -> str:
    """the text under a placed line, rebuilt from SEQ, CIGAR and MD alone (M, I and D operations)"""
    assert MD_RE.match(md), md
    # SEQ without its inserted bases: what MD speaks about
    aligned, i = [], 0
    ops = re.findall(r"(\d+)([MID])", cigar)
    assert "".join(a + b for a, b in ops) == cigar, cigar
    for num, op in ops:
        if op == "M":
            aligned.append(seq[i:i + int(num)])
            i += int(num)
        elif op == "I":
            i += int(num)
    assert i == len(seq), (i, len(seq), cigar)
    aligned = "".join(aligned)
    ref, i = [], 0
    for num, dele, sub in re.findall(r"(\d+)|\^([A-Z]+)|([A-Z])", md):
        if num:
            ref.append(aligned[i:i + int(num)])
            i += int(num)
        elif dele:
            ref.append(dele)
        else:
            ref.append(sub)
            i += 1
    assert i == len(aligned), (i, len(aligned), md)
    ref = "".join(ref)
    assert len(ref) == sum(int(a) for a, b in ops if b in "MD")
    return ref


# ---- the SAM text of `real -sam ... -gapped ... -sam_gapped 1` ---------------------------------------------------------------
def sam_pairs_gapped(genomes, b1, b2, pairs, s1, s2, gaps, min_ins: int, max_ins: int, scores: bool, fastq=(True, True)):
    """-> (the whole file, the per-file counters of the gapped lists).  sam_checker.sam_pairs' file, except that a fragment whose
    gap record is Unique has, in the pass of the record's file (the anchor's), two placed lines"""
    plain, _ = sk.sam_pairs(genomes, b1, b2, pairs, s1, s2, scores, fastq)
    fin = sk.final_pairs(pairs, s1, s2)
    bs = (b1, b2)
    lines = plain.split("\n")[:-1]
    n_head = sum(1 for l in lines if l.startswith("@"))
    # the plain file's lines, keyed as sam_pairs writes them: per file, per fragment, per mate
    k, at = n_head, {}
    for fi in range(len(genomes)):
        for i in range(b1.n_reads):
            for m in (0, 1):
                j, o = 2 * i + m, 2 * i + 1 - m
                here = fin.placed[j] and int(fin.fileid[j]) == fi
                beside = not fin.placed[j] and fin.placed[o] and int(fin.fileid[o]) == fi
                nothing = not fin.placed[j] and not fin.placed[o] and fi == len(genomes) - 1
                if here or beside or nothing:
                    at[(fi, i, m)] = k
                    k += 1
    assert k == len(lines)
    ctrs = []
    for fi, g in enumerate(genomes):
        # the records as they stand when the pass of file fi lists them: those of later files are still NoMatch
        seen = gaps.copy()
        later = (gc.state_of(seen["tag"]) != gc.NOMATCH) & (seen["fileid"] > fi)
        seen[later] = gc.empty_records(int(later.sum()))
        lists, off, ctr = gapped_lists(g.sym, fi, b1, b2, seen)
        ctrs.append(ctr)
        for i in range(b1.n_reads):
            rec = gaps[i]
            if int(gc.state_of(rec["tag"])) != gc.UNIQUE or int(rec["fileid"]) != fi:
                continue
            t = int(gc.target_of(rec["tag"]))
            a = 1 - t
            ja = 2 * i + a
            assert fin.placed[ja] and not fin.placed[2 * i + t] and int(fin.fileid[ja]) == fi
            lt = int(bs[t].offsets[i + 1]) - int(bs[t].offsets[i])
            la = int(bs[a].offsets[i + 1]) - int(bs[a].offsets[i])
            gap = int(rec["gap"])
            tinv, ainv = bool(gc.inverted_of(rec["tag"])), bool(fin.inv[ja])
            tpos, apos = int(rec["pos"]), int(fin.pos[ja])
            span = lt + gap
            # the outer distance: from the forward mate's first base to the reverse mate's last
            outer = (tpos + span - apos) if tinv else (apos + la - tpos)
            assert tinv != ainv
            proper = min_ins <= outer <= max_ins
            gt = genomes[int(rec["fileid"])]
            tname, tpos1 = sk.frag_name(gt.frag_names[int(rec["frag"])]), tpos - int(gt.frag_start[int(rec["frag"])]) + 1
            aname, apos1 = sk._where(genomes, fin, ja)
            same = int(rec["frag"]) == int(fin.frag[ja])
            # the anchor's line: FLAG, RNEXT, PNEXT, TLEN change
            f = lines[at[(fi, i, a)]].split("\t")
            flag = (int(f[1]) & ~8) | (32 if tinv else 0) | (2 if proper else 0)
            f[1], f[6], f[7], f[8] = str(flag), "=" if same else tname, str(tpos1), str(-outer if ainv else outer)
            lines[at[(fi, i, a)]] = "\t".join(f)
            # the rescued mate's line
            L = lists[int(off[i]):int(off[i + 1])]
            seq, qual = sk._seq_qual(bs[t], i, tinv, fastq[t])
            flag = 1 | (64 if t == 0 else 128) | (16 if tinv else 0) | (32 if ainv else 0) | (2 if proper else 0)
            lines[at[(fi, i, t)]] = "\t".join([sk.qname(bs[t].ids[i], True), str(flag), tname, str(tpos1), "255", gc.cigar_of(rec, lt), "=" if same else aname,
                                               str(apos1), str(-outer if tinv else outer), seq, qual, "NM:i:%d" % nm_of(L, gap),
                                               "MD:Z:" + md_of(L, span), "ZC:i:%d" % int(rec["cost"])])
    return "\n".join(lines) + "\n", ctrs


def stderr_line(ctrs) -> str:
    return "sam gapped: mates=%d deleted=%d inserted=%d disagree=%d" % tuple(sum(c[k] for c in ctrs) for k in ("placed", "deleted", "inserted", "disagree"))
