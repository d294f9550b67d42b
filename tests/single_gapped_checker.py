"""What a single-end run with the gapped consumers writes (`real -gapped_single g.tsv -sam_gapped 1 -pileup_gapped 1 -vcf_indels 1
[-dedup 1]`) -- TEST INFRASTRUCTURE ONLY.  Composed from the checkers of the parts: sam_checker and
gapped_list_checker for the -sam text, pileup_gapped_checker and indel_checker -- the batch given as both mates -- for the
pileup, the calls and the indel calls, dup_gapped_checker for the marks.  It never calls the code under test."""
from __future__ import annotations

import numpy as np

import dup_checker as dk
import dup_gapped_checker as dgk
import gap_checker as gc
import gapped_list_checker as glk
import indel_checker as ic
import pileup_gapped_checker as pgc
import sam_checker as sk


def sam_single_gapped(genomes, b, info, gaps, dup=None, fastq: bool = True):
    """-> (the whole -sam file, the per-file counters of the gapped lists).  sam_checker.sam_single's file (scores off), except
    that a read whose info word places nothing and whose gap record is Unique has ONE line, as placed, in the pass of the record's
    file -- FLAG 0 / 16, the record's CIGAR, MAPQ 255, no mate fields, NM / MD from its gapped list, ZC -- and none as unplaced in
    the last pass; dup: the marks, 1024 on the line of a marked read"""
    fin = sk.final_single(info, None)
    n = b.n_reads
    dup = np.zeros(n, dtype=np.uint8) if dup is None else np.asarray(dup)
    out, ctrs = [sk.header(genomes)], []
    unique = gc.state_of(gaps["tag"]) == gc.UNIQUE
    for fi, g in enumerate(genomes):
        lists, off, _ = sk.mismatch_lists(g.sym, fi, fin, sk.single_reads(b))
        glists, goff, ctr = glk.gapped_lists(g.sym, fi, b, b, gaps)
        ctrs.append(ctr)
        for i in range(n):
            q = sk.qname(b.ids[i], False)
            L = int(b.offsets[i + 1]) - int(b.offsets[i])
            mark = 1024 if dup[i] else 0
            if fin.placed[i]:
                if int(fin.fileid[i]) != fi:
                    continue
                seq, qual = sk._seq_qual(b, i, bool(fin.inv[i]), fastq)
                name, pos = sk._where(genomes, fin, i)
                out.append("\t".join([q, str((16 if fin.inv[i] else 0) + mark), name, str(pos), "255", "%dM" % L, "*", "0", "0", seq, qual] +
                                     sk._tags(lists[int(off[i]):int(off[i + 1])], L, 0.0, False)) + "\n")
            elif unique[i]:
                rec = gaps[i]
                if int(rec["fileid"]) != fi:
                    continue
                inv = bool(gc.inverted_of(rec["tag"]))
                gg = genomes[fi]
                gl = glists[int(goff[i]):int(goff[i + 1])]
                seq, qual = sk._seq_qual(b, i, inv, fastq)
                out.append("\t".join([q, str((16 if inv else 0) + mark), sk.frag_name(gg.frag_names[int(rec["frag"])]),
                                      str(int(rec["pos"]) - int(gg.frag_start[int(rec["frag"])]) + 1), "255", gc.cigar_of(rec, L), "*", "0", "0", seq, qual,
                                      "NM:i:%d" % glk.nm_of(gl, int(rec["gap"])), "MD:Z:" + glk.md_of(gl, L + int(rec["gap"])), "ZC:i:%d" % int(rec["cost"])]) + "\n")
            elif fi == len(genomes) - 1:
                assert not mark
                seq, qual = sk._seq_qual(b, i, False, fastq)
                out.append("\t".join([q, "4", "*", "0", "0", "*", "*", "0", "0", seq, qual]) + "\n")
    return "".join(out), ctrs


def sam_gapped_line(ctrs) -> str:
    return "sam gapped: reads=%d deleted=%d inserted=%d disagree=%d" % tuple(sum(c[k] for c in ctrs) for k in ("placed", "deleted", "inserted", "disagree"))


def file_expected(g, fid, b, info, gaps, dup=None, min_qual: int = 20, pileup_gapped: bool = True):
    """(pileup, SNP calls, indel calls) of genome file `fid` of a single-end run: the info words piled up, the Unique gap records
    behind them (the batch as both mates), the same as evidence at the sites, the records' indels over the finished pileup;
    dup: the marked reads are left out of all of it -- an info word as NoMatch, a gap record as the NoMatch record"""
    if dup is not None:
        info, gaps = dk.masked_info(info, dup), dgk.masked_gaps(gaps, dup)
    pu = pgc.GappedPileup(g.sym, fid, min_qual)
    pu.add(b, info)
    if pileup_gapped:
        pu.add_gapped(b, b, gaps)
    cl = pgc.GappedCalls(pu)
    cl.add(b, info)
    if pileup_gapped:
        cl.add_gapped(b, b, gaps)
    ind = ic.Indels(pu.ungapped_view(), g.frag_start)
    ind.add(b, b, gaps)
    return pu, cl, ind
