"""The indel calls restated in numpy -- TEST INFRASTRUCTURE ONLY (include/real_hip.h, "indel calls"): events from gap records,
the left-normalisation in two formulations, groups, genotypes, the two lists, every counter, the VCF lines and the stderr line
of `real -vcf_indels 1`, on top of gapped_list_checker (which records fit, the oriented read) and a FINISHED
pileup_checker.Pileup (depth, min_qual).  It never calls the code under test and imports nothing of the product.  Everything is
an integer or a string."""
from __future__ import annotations

import numpy as np

import call_checker as ck
import gap_checker as gc
import gapped_list_checker as glc
import pileup_checker as pk

SHIFT_MAX, REF_Q, PRIOR_HET, PRIOR_HOM, HET = 256, 30, 40, 43, 3          # REAL_HIP_INDEL_*, REAL_HIP_CALL_HET
INDEL_DTYPE = np.dtype([("pos", "<u4"), ("ref_n", "<u4"), ("alt_n", "<u4"), ("alt_fwd", "<u4"), ("qsum", "<u4"), ("qual", "<u4"), ("seq", "<u4"),
                        ("gap", "i1"), ("gt", "u1"), ("gq", "u1"), ("ref", "u1")])
assert INDEL_DTYPE.itemsize == 32
COUNTERS = ("fragments", "placed", "other_file", "invalid", "ungapped", "events", "on_n", "low_qual", "shifted", "shift_capped")


def pack_seq(s) -> int:
    """S as the record holds it: 2 bits a base, the first base lowest"""
    return sum(int(b) << (2 * k) for k, b in enumerate(s))


def unpack_seq(seq: int, d: int):
    return [(int(seq) >> (2 * k)) & 3 for k in range(d)]


# ---- the left-normalisation, twice -------------------------------------------------------------------------------------------
def shift_loop(sym, fs: int, x: int, g: int, s):
    """the definition: one base at a time -> (x, S, shifts, capped)"""
    sym = np.asarray(sym)
    s = [int(b) for b in s]
    d = len(s)
    ref = lambda i: 0 if sym[i] > 3 else int(sym[i])                     # noqa: E731 (the 2-bit text stores an N as 0)

    def may(x):
        if not (x - 1 > fs and sym[x - 1] <= 3 and sym[x - 2] <= 3):
            return False
        return ref(x - 1) == ref(x + g - 1) if g > 0 else ref(x - 1) == s[d - 1]
    n = 0
    while n < SHIFT_MAX and may(x):
        if g < 0:
            s = [ref(x - 1)] + s[:d - 1]
        x -= 1
        n += 1
    return x, s, n, n == SHIFT_MAX and may(x)


def shift_run(sym, fs: int, x: int, g: int, s):
    """the same from the run, ending at x, of positions i with T'[i] == T'[i + |g|]: T' is the text for a deletion, and the text
    in front of x followed by S for an insertion"""
    sym = np.asarray(sym)
    ag, d = abs(g), max(-g, 0)
    lo = max(fs, x - SHIFT_MAX - 2)                                        # the window [lo, x + ag) of T'
    t = np.where(sym[lo:x + ag] > 3, 0, sym[lo:x + ag]).astype(np.int64) if g > 0 else \
        np.concatenate([np.where(sym[lo:x] > 3, 0, sym[lo:x]), np.asarray(s, dtype=np.int64)]).astype(np.int64)
    i = np.arange(lo + 1, x)                                               # the positions a step may go to: i > fs, and i - 1 >= lo
    ok = (i > fs) & (sym[i] <= 3) & (sym[i - 1] <= 3) & (t[i - lo] == t[i - lo + ag])
    bad = np.nonzero(~ok[::-1])[0]
    run = int(bad[0]) if bad.size else int(ok.shape[0])                    # (all good: the window's SHIFT_MAX + 1, or down to fs + 1)
    n = min(run, SHIFT_MAX)
    xf = x - n
    return xf, [int(v) for v in t[xf - lo:xf - lo + d]], n, run > SHIFT_MAX


# ---- genotypes ---------------------------------------------------------------------------------------------------------------
def likelihoods(alt_n: int, ref_n: int, qsum: int):
    return [int(qsum), HET * (int(ref_n) + int(alt_n)) + PRIOR_HET, REF_Q * int(ref_n) + PRIOR_HOM]


def genotype(alt_n: int, ref_n: int, qsum: int):
    """-> (best 0 / 1 / 2, QUAL, GQ): the first of minimal PL in the order 0/0, 0/1, 1/1"""
    pl = likelihoods(alt_n, ref_n, qsum)
    best = min(range(3), key=lambda k: (pl[k], k))
    return best, min(pl[0] - pl[best], 0xffffffff), min(99, min(pl[k] for k in range(3) if k != best) - pl[best])


# ---- the stage ---------------------------------------------------------------------------------------------------------------
class Indels:
    """the events over a finished pk.Pileup (same text, file id and min_qual) of a text with the fragments frag_start"""

    def __init__(self, pu: pk.Pileup, frag_start, shift=shift_loop):
        self.pu, self.fs, self.shift = pu, [int(v) for v in frag_start], shift
        self.stats = dict.fromkeys(COUNTERS, 0)
        self.groups = {}                                                  # (x, g, seq) -> [alt_n, alt_fwd, qsum]
        self.raw = []                                                     # (fragment index in its add, x0, g, x, seq) per event, for the tests

    def event_of(self, rec, read, qual):
        """one Unique record of this file -> None, or (x, g, S, q, forward) after the N and quality drops and the shift"""
        sym, st = self.pu.sym, self.stats
        l = int(read.shape[0])
        frag, p, g, j = int(rec["frag"]), int(rec["pos"]), int(rec["gap"]), int(rec["split"])
        fits = glc.fits(rec, l, self.pu.n) and frag < len(self.fs) - 1
        if fits:
            fs, fe = self.fs[frag], self.fs[frag + 1]
            fits = fs <= p and p + l + g <= fe
        if not fits:
            st["invalid"] += 1
            return None
        st["placed"] += 1
        if g == 0:
            st["ungapped"] += 1
            return None
        inv = bool(gc.inverted_of(rec["tag"]))
        r = gc.oriented(read, inv)
        d = max(-g, 0)
        x = p + j
        if (sym[x - 1:x + max(g, 0)] > 3).any():
            st["on_n"] += 1
            return None
        q = 30
        if qual is not None:
            qo = np.asarray(qual)[::-1] if inv else np.asarray(qual)
            q = int(qo[j - 1:j + d + 1].min())
        if q < self.pu.min_qual:
            st["low_qual"] += 1
            return None
        xf, s, n, capped = self.shift(sym, fs, x, g, [int(b) for b in r[j:j + d]])
        st["shifted"] += n > 0
        st["shift_capped"] += bool(capped)
        return xf, g, s, q, not inv

    def add(self, b1, b2, gaps):
        n = int(gaps.shape[0])
        self.stats["fragments"] += n
        for i in range(n):
            rec = gaps[i]
            if int(gc.state_of(rec["tag"])) != gc.UNIQUE:
                continue
            if int(rec["fileid"]) != self.pu.fileid:
                self.stats["other_file"] += 1
                continue
            b = (b1, b2)[int(gc.target_of(rec["tag"]))]
            lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
            ev = self.event_of(rec, b.bases[lo:hi], None if b.qual is None else b.qual[lo:hi])
            if ev is None:
                continue
            x, g, s, q, fwd = ev
            self.stats["events"] += 1
            acc = self.groups.setdefault((x, g, pack_seq(s)), [0, 0, 0])
            acc[0] += 1
            acc[1] += int(fwd)
            acc[2] += q
            self.raw.append((i, int(rec["pos"]) + int(rec["split"]), g, x, pack_seq(s)))

    def events(self, min_call_qual: int = 20, min_alt: int = 2, min_depth: int = 4):
        """the event list under the thresholds: ascending (x, g, S), gt = the decision"""
        keys = sorted(self.groups)
        out = np.zeros(len(keys), dtype=INDEL_DTYPE)
        for k, (x, g, seq) in enumerate(keys):
            alt_n, alt_fwd, qsum = self.groups[(x, g, seq)]
            ref_n = int(min(self.pu.depth[x - 1], self.pu.depth[x]))
            best, qual, gq = genotype(alt_n, ref_n, qsum)
            call = best != 0 and qual >= min_call_qual and alt_n >= min_alt and ref_n + alt_n >= min_depth
            out[k] = (x - 1, ref_n, alt_n, alt_fwd, qsum, qual, seq, g, best if call else 0, gq, int(self.pu.ref[x - 1]))
        return out

    def calls(self, min_call_qual: int = 20, min_alt: int = 2, min_depth: int = 4):
        e = self.events(min_call_qual, min_alt, min_depth)
        return e[e["gt"] != 0]

    def finish_stats(self, min_call_qual: int = 20, min_alt: int = 2, min_depth: int = 4):
        """every field of real_hip_indel_stats but launches and kernel_ms"""
        c = self.calls(min_call_qual, min_alt, min_depth)
        return dict(self.stats, distinct=len(self.groups), calls=int(c.shape[0]), het=int((c["gt"] == 1).sum()), hom=int((c["gt"] == 2).sum()),
                    deletions=int((c["gap"] > 0).sum()), insertions=int((c["gap"] < 0).sum()))


def assert_lists_equal(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: %d records, want %d" % (what, got.shape[0], want.shape[0])
    bad = np.nonzero((got.view(np.uint8).reshape(-1, 32) != want.view(np.uint8).reshape(-1, 32)).any(axis=1))[0]
    assert bad.size == 0, "%s: %d records differ, first %d: got %r want %r" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


# ---- what `real -vcf ... -vcf_indels 1` writes ---------------------------------------------------------------------------------
INDEL_INFO = ['##INFO=<ID=INDEL,Number=0,Type=Flag,Description="An insertion or deletion shown by gap-rescued mates">\n',
              '##INFO=<ID=SF,Number=1,Type=Integer,Description="Supporting mates on the forward strand">\n',
              '##INFO=<ID=SR,Number=1,Type=Integer,Description="Supporting mates on the reverse strand">\n']


def vcf_header(contigs):
    """call_checker.vcf_header with the three ##INFO lines of the indels behind DP's"""
    lines = ck.vcf_header(contigs).splitlines(keepends=True)
    at = max(k for k, l in enumerate(lines) if l.startswith("##INFO")) + 1
    return "".join(lines[:at] + INDEL_INFO + lines[at:])


def vcf_line(c, sym, frag_start, frag_names) -> str:
    fs = np.asarray(frag_start, dtype=np.int64)
    a, g = int(c["pos"]), int(c["gap"])
    f = int(np.searchsorted(fs, a, side="right")) - 1
    anchor = "ACGT"[int(c["ref"])]
    if g > 0:
        ref, alt = anchor + "".join("ACGT"[int(v)] for v in sym[a + 1:a + 1 + g]), anchor
    else:
        ref, alt = anchor, anchor + "".join("ACGT"[v] for v in unpack_seq(int(c["seq"]), -g))
    ref_n, alt_n, fwd = int(c["ref_n"]), int(c["alt_n"]), int(c["alt_fwd"])
    return "%s\t%d\t.\t%s\t%s\t%d\t.\tDP=%d;INDEL;SF=%d;SR=%d\tGT:GQ:DP:AD\t%s:%d:%d:%d,%d\n" % (
        frag_names[f], a - int(fs[f]) + 1, ref, alt, int(c["qual"]), ref_n + alt_n, fwd, alt_n - fwd, ("0/1", "1/1")[int(c["gt"]) - 1], int(c["gq"]),
        ref_n + alt_n, ref_n, alt_n)


def vcf_lines_merged(snp_calls, indel_calls, sym, frag_start, frag_names) -> str:
    """the lines of one genome file: SNP calls and indel calls merged by text position, the SNP first at an equal one"""
    rows = [(int(c["pos"]), 0, k, ck.vcf_lines(snp_calls[k:k + 1], frag_start, frag_names)) for k, c in enumerate(snp_calls)]
    rows += [(int(c["pos"]), 1, k, vcf_line(c, sym, frag_start, frag_names)) for k, c in enumerate(indel_calls)]
    return "".join(r[3] for r in sorted(rows, key=lambda r: r[:3]))


def stderr_line(ind: Indels, name: str, min_call_qual: int = 20, min_alt: int = 2, min_depth: int = 4) -> str:
    st = ind.finish_stats(min_call_qual, min_alt, min_depth)
    return "indels: file=%s events=%d distinct=%d calls=%d het=%d hom=%d deletions=%d insertions=%d shifted=%d low_qual=%d" % (
        name, st["events"], st["distinct"], st["calls"], st["het"], st["hom"], st["deletions"], st["insertions"], st["shifted"], st["low_qual"])
