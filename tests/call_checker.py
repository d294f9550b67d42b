"""The variant calls restated in numpy -- TEST INFRASTRUCTURE ONLY (include/real_hip.h, "variant calls"): evidence, genotypes,
calls, the VCF lines and the stderr line of `real -vcf`, on top of a FINISHED pileup_checker.Pileup.  It is fed the ORACLE's
records and never calls the code under test.  Everything is an integer."""
from __future__ import annotations

import numpy as np

import pileup_checker as pk

HET, ERR, PRIOR_HET, PRIOR_HOM, PRIOR_HET2 = 3, 5, 30, 33, 60          # REAL_HIP_CALL_*
EVIDENCE_DTYPE = np.dtype([("cnt", "<u4", (4,)), ("qsum", "<u4", (4,))])
CALL_DTYPE = np.dtype([("pos", "<u4"), ("depth", "<u4"), ("cnt", "<u4", (4,)), ("qual", "<u4"), ("ref", "u1"), ("a1", "u1"), ("a2", "u1"), ("gq", "u1")])
COUNTERS = ("reads", "placed", "other_file", "invalid", "site_bases", "low_qual")


def genotype_order(ref: int):
    """the ten genotypes in the order ties are broken by: (ref, ref) first, then the other nine by ascending (a, b)"""
    return [(ref, ref)] + [(a, b) for a in range(4) for b in range(a, 4) if not (a == b == ref)]


def likelihoods(ref: int, cnt, qsum):
    """the ten PLs of one site, in genotype_order(ref)"""
    cnt, qsum = [int(v) for v in cnt], [int(v) for v in qsum]
    E = [qsum[d] + ERR * cnt[d] for d in range(4)]
    out = []
    for a, b in genotype_order(ref):
        if a == b:
            pl = sum(E[d] for d in range(4) if d != a) + (0 if a == ref else PRIOR_HOM)
        else:
            pl = HET * (cnt[a] + cnt[b]) + sum(E[d] for d in range(4) if d not in (a, b)) + (PRIOR_HET if ref in (a, b) else PRIOR_HET2)
        out.append(pl)
    return out


def genotype(ref: int, cnt, qsum):
    """-> (a1, a2, QUAL, GQ) of one site: the first genotype of minimal PL"""
    order, pl = genotype_order(ref), likelihoods(ref, cnt, qsum)
    best = min(range(10), key=lambda k: (pl[k], k))
    others = [pl[k] for k in range(10) if k != best]
    return order[best][0], order[best][1], min(pl[0] - pl[best], 0xffffffff), min(99, min(others) - pl[best])


class Calls:
    """the evidence over the sites of a finished pk.Pileup (same text, file id and min_qual), and the calls from it"""

    def __init__(self, pu: pk.Pileup):
        self.pu = pu
        self.site_list = pu.sites()
        self.slot = np.full(pu.n, -1, dtype=np.int64)
        self.slot[self.site_list["pos"].astype(np.int64)] = np.arange(self.site_list.shape[0])
        self.cnt = np.zeros((self.site_list.shape[0], 4), dtype=np.int64)
        self.qsum = np.zeros((self.site_list.shape[0], 4), dtype=np.int64)
        self.stats = {k: 0 for k in COUNTERS}

    def place(self, read, qual, p: int, inverted: bool):
        read = np.asarray(read, dtype=np.int64)
        L = int(read.shape[0])
        if p + L > self.pu.n:
            self.stats["invalid"] += 1
            return
        q = np.full(L, 30, dtype=np.int64) if qual is None else np.asarray(qual, dtype=np.int64)
        if inverted:
            read, q = 3 - read[::-1], q[::-1]
        self.stats["placed"] += 1
        s = self.slot[p:p + L]
        at = s >= 0
        good = at & (q >= self.pu.min_qual)
        self.stats["low_qual"] += int((at & ~good).sum())
        self.stats["site_bases"] += int(good.sum())
        np.add.at(self.cnt, (s[good], read[good]), 1)
        np.add.at(self.qsum, (s[good], read[good]), q[good])

    def add(self, b, info):
        info = np.asarray(info, dtype=np.uint64)
        state = (info >> np.uint64(61)).astype(np.int64)
        fileid = ((info >> np.uint64(35)) & np.uint64(63)).astype(np.int64)
        pos = (info & np.uint64((1 << 35) - 1)).astype(np.int64)
        self.stats["reads"] += int(info.shape[0])
        for i in np.nonzero((state == 1) | (state == 2))[0]:
            if fileid[i] != self.pu.fileid:
                self.stats["other_file"] += 1
                continue
            self.place(*self.pu._read(b, i), int(pos[i]), state[i] == 2)

    def add_pairs(self, b1, b2, pairs):
        self.stats["reads"] += 2 * int(pairs.shape[0])
        for i in np.nonzero(pairs["state"] == pk.UNIQUE)[0]:
            if int(pairs["fileid"][i]) != self.pu.fileid:
                self.stats["other_file"] += 2
                continue
            inv1 = bool(pairs["inverted1"][i])
            self.place(*self.pu._read(b1, i), int(pairs["pos1"][i]), inv1)
            self.place(*self.pu._read(b2, i), int(pairs["pos2"][i]), not inv1)

    def evidence(self):
        e = np.zeros(self.cnt.shape[0], dtype=EVIDENCE_DTYPE)
        e["cnt"], e["qsum"] = self.cnt, self.qsum
        return e

    def genotypes(self):
        """the best genotype of every site as CALL_DTYPE records, whatever the thresholds (computed once: call it after the adds)"""
        if getattr(self, "_gt", None) is None:
            g = np.zeros(self.site_list.shape[0], dtype=CALL_DTYPE)
            g["pos"], g["depth"], g["cnt"], g["ref"] = self.site_list["pos"], self.site_list["depth"], self.cnt, self.site_list["ref"]
            for s in range(g.shape[0]):
                g["a1"][s], g["a2"][s], g["qual"][s], g["gq"][s] = genotype(int(g["ref"][s]), self.cnt[s], self.qsum[s])
            self._gt = g
        return self._gt

    def calls(self, min_call_qual: int = 20, min_depth: int = 4):
        g = self.genotypes()
        variant = (g["a1"] != g["ref"]) | (g["a2"] != g["ref"])
        return g[variant & (g["qual"] >= min_call_qual) & (self.cnt.sum(axis=1) >= min_depth)]

    def finish_stats(self, min_call_qual: int = 20, min_depth: int = 4):
        """every field of real_hip_call_stats but launches and kernel_ms"""
        c = self.calls(min_call_qual, min_depth)
        het = int((c["a1"] != c["a2"]).sum())
        return dict(self.stats, calls=int(c.shape[0]), het=het, hom=int(c.shape[0]) - het)


# ---- what `real -vcf` writes ---------------------------------------------------------------------------------------
def vcf_header(contigs):
    """contigs: [(fragment name, length)] of all genome files in order"""
    out = ["##fileformat=VCFv4.2\n"]
    out += ["##contig=<ID=%s,length=%d>\n" % (name, length) for name, length in contigs]
    out += ['##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth of the placements, no quality filter">\n',
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n',
            '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">\n',
            '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Bases of sufficient quality">\n',
            '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Bases of sufficient quality per allele">\n',
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n"]
    return "".join(out)


def vcf_lines(calls, frag_start, frag_names):
    out = []
    fs = np.asarray(frag_start, dtype=np.int64)
    for c in calls:
        f = int(np.searchsorted(fs, int(c["pos"]), side="right")) - 1
        ref = int(c["ref"])
        alts = sorted({int(c["a1"]), int(c["a2"])} - {ref})
        alleles = [ref] + alts
        out.append("%s\t%d\t.\t%s\t%s\t%d\t.\tDP=%d\tGT:GQ:DP:AD\t%d/%d:%d:%d:%s\n" % (
            frag_names[f], int(c["pos"]) - int(fs[f]) + 1, "ACGT"[ref], ",".join("ACGT"[a] for a in alts), int(c["qual"]), int(c["depth"]),
            *sorted((alleles.index(int(c["a1"])), alleles.index(int(c["a2"])))), int(c["gq"]), int(c["cnt"].sum()), ",".join(str(int(c["cnt"][a])) for a in alleles)))
    return "".join(out)


def stderr_line(cl: Calls, name: str, min_call_qual: int = 20, min_depth: int = 4):
    st = cl.finish_stats(min_call_qual, min_depth)
    return "calls: file=%s sites=%d calls=%d het=%d hom=%d site_bases=%d low_qual=%d" % (
        name, cl.site_list.shape[0], st["calls"], st["het"], st["hom"], st["site_bases"], st["low_qual"])
