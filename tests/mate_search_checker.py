"""The checker of the mate-search tests -- TEST INFRASTRUCTURE ONLY.

A brute-force statement of the semantics in include/real_hip.h ("mate search"): for every anchor every position of its
window is tested with numpy on the genome's symbols (Hamming distance) and with the oracle's own predicates and scorer
(ora_is_position_valid, ora_is_dontcare_free, ora_position_to_range, ora_compute_score).  The extra candidates go
through pairs_checker.record_of / merge.  It never calls the code under test and imports nothing of the product.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import pairs_checker as pc

COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
MAX_PATL = 320
COUNTERS = ("anchors", "anchors_skipped", "positions", "placements")


def read_of(b, i):
    lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
    return b.bases[lo:hi], (None if b.qual is None else b.qual[lo:hi])


def eligible(read, seedl):
    """what the matcher does not skip (and the search can hold)"""
    return seedl <= len(read) <= MAX_PATL and not (read > 3).any()


def oriented(read, inverted):
    return COMP[read[::-1]] if inverted else read


def window_of(pa, la, lb, inverted, fs, fe, min_ins, max_ins):
    """positions p of the other mate (length lb, opposite strand) concordant with the anchor at pa (length la) and wholly
    inside the anchor's fragment [fs, fe): inclusive bounds, lo > hi if empty"""
    if not inverted:        # the anchor is the forward mate
        lo = max(pa, pa + la - lb, pa + min_ins - lb)
        hi = min(pa + max_ins - lb, fe - lb)
    else:
        lo = max(pa + la - max_ins, fs)
        hi = min(pa, pa + la - lb, pa + la - min_ins)
    return lo, hi


class Searcher:
    """one genome file: the symbols, the oracle's genome (validity, score) and the parameters of the run"""

    def __init__(self, ora, g, seedl, totalkmax, scores, min_ins, max_ins, max_anchors=0, LL=None):
        self.ora, self.g = ora, g
        self.og = ora.Genome(g.sym, g.frag_start)
        self.L = ora.lib()
        self.seedl, self.kmax, self.scores = seedl, totalkmax, bool(scores)
        self.min_ins, self.max_ins, self.max_anchors = min_ins, max_ins, max_anchors
        self.LL = np.ascontiguousarray(ora.scoring_table()[0] if LL is None else LL, dtype=np.float64)
        self.fs = np.asarray(g.frag_start, dtype=np.int64)

    def placement(self, read, qual, inverted, p):
        """(k, score, frag) of the read on that strand at p, or None"""
        lb = len(read)
        if p < 0 or p + lb > self.g.sym.shape[0]:
            return None
        if not self.L.ora_is_position_valid(self.og.h, p, lb) or not self.L.ora_is_dontcare_free(self.og.h, p, lb):
            return None
        k = int((self.g.sym[p:p + lb] != oriented(read, inverted)).sum())
        if k > self.kmax:
            return None
        sc = np.float32(1.0)
        if self.scores:
            rd = np.ascontiguousarray(read, dtype=np.uint8)
            q = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint8)
            sc = np.float32(self.L.ora_compute_score(self.og.h, self.LL.ctypes.data_as(C.c_void_p), int(inverted), rd.ctypes.data_as(C.c_void_p),
                                                     None if q is None else q.ctypes.data_as(C.c_void_p), p, lb))
        return k, sc, int(self.L.ora_position_to_range(self.og.h, p))

    def candidate(self, fileid, m, a, p, pl):
        """the pair (anchor a of mate m, placement pl of the other mate at p) in pairs_checker's candidate form"""
        k, sc, frag = pl
        assert frag == int(a["frag"])
        sa, ka, inva = np.float32(a["score"]), int(a["k"]), int(bool(a["inverted"]))
        if m == 0:
            s1, s2, k1, k2, pos1, pos2, inv1 = sa, sc, ka, k, int(a["pos"]), p, inva
        else:
            s1, s2, k1, k2, pos1, pos2, inv1 = sc, sa, k, ka, p, int(a["pos"]), 1 - inva
        v = float(np.float64(s1) + np.float64(s2)) if self.scores else -float(k1 + k2)
        return v, (int(fileid), frag, pos1, pos2, inv1), (s1, s2, k1, k2)

    def extras(self, fileid, r1, q1, r2, q2, h1, h2, counters):
        """the candidates the search adds for one fragment: anchors h1 (mate 1) and h2 (mate 2)"""
        out = []
        reads = ((r1, q1), (r2, q2))
        if not (eligible(r1, self.seedl) and eligible(r2, self.seedl)):
            return out
        for m, hits in enumerate((h1, h2)):
            if self.max_anchors and len(hits) > self.max_anchors:
                counters["anchors_skipped"] += len(hits)
                continue
            rb, qb = reads[1 - m]
            la, lb = len(reads[m][0]), len(rb)
            for a in hits:
                f, pa, inva = int(a["frag"]), int(a["pos"]), bool(a["inverted"])
                fs, fe = int(self.fs[f]), int(self.fs[f + 1])
                assert fs <= pa and pa + la <= fe, "an anchor lies inside its fragment"
                counters["anchors"] += 1
                lo, hi = window_of(pa, la, lb, inva, fs, fe, self.min_ins, self.max_ins)
                if lo > hi:
                    continue
                counters["positions"] += hi - lo + 1
                ob = oriented(rb, not inva)
                win = np.lib.stride_tricks.sliding_window_view(self.g.sym[lo:hi + lb], lb)
                for j in np.nonzero((win != ob[None, :]).sum(axis=1) <= self.kmax)[0]:
                    p = lo + int(j)
                    pl = self.placement(rb, qb, not inva, p)
                    if pl is not None:
                        counters["placements"] += 1
                        out.append(self.candidate(fileid, m, a, p, pl))
        return out


def check_pairs_search(ora, genomes, files, b1, b2, min_ins, max_ins, scores, filter_mult, seedl, totalkmax, max_anchors=0, search=True):
    """genomes: {fileid: synth.Genome}; files: [(fileid, hits1, off1, hits2, off2)] (oracle match_all lists or hand-made
    anchors); -> (records over the union of the files, the four counters).  search=False: pairs_checker.check_pairs."""
    n = b1.n_reads
    out = np.zeros(n, dtype=pc.REC_DTYPE)
    counters = {k: 0 for k in COUNTERS}
    S = {fid: Searcher(ora, genomes[fid], seedl, totalkmax, scores, min_ins, max_ins, max_anchors) for fid, *_ in files}
    for i in range(n):
        (r1, q1), (r2, q2) = read_of(b1, i), read_of(b2, i)
        cands = []
        for fid, h1, o1, h2, o2 in files:
            a1, a2 = h1[int(o1[i]):int(o1[i + 1])], h2[int(o2[i]):int(o2[i + 1])]
            cands += pc.candidates(a1, a2, len(r1), len(r2), min_ins, max_ins, scores, fid)
            if search:
                cands += S[fid].extras(fid, r1, q1, r2, q2, a1, a2, counters)
        out[i] = pc.record_of(cands, pc.eps_of(scores, filter_mult, len(r1), len(r2)))
    return out, counters


def search_only(ora, genomes, files, b1, b2, min_ins, max_ins, scores, filter_mult, seedl, totalkmax, max_anchors=0):
    """what real_hip_pair_search alone folds into fresh records: the pairs (anchor, placement), not the join"""
    n = b1.n_reads
    out = np.zeros(n, dtype=pc.REC_DTYPE)
    counters = {k: 0 for k in COUNTERS}
    S = {fid: Searcher(ora, genomes[fid], seedl, totalkmax, scores, min_ins, max_ins, max_anchors) for fid, *_ in files}
    for i in range(n):
        (r1, q1), (r2, q2) = read_of(b1, i), read_of(b2, i)
        cands = []
        for fid, h1, o1, h2, o2 in files:
            cands += S[fid].extras(fid, r1, q1, r2, q2, h1[int(o1[i]):int(o1[i + 1])], h2[int(o2[i]):int(o2[i + 1])], counters)
        out[i] = pc.record_of(cands, pc.eps_of(scores, filter_mult, len(r1), len(r2)))
    return out, counters


def whole_genome_pairs(ora, g, fileid, f, b1, b2, min_ins, max_ins, scores, filter_mult, seedl, totalkmax, max_anchors=0):
    """A second, differently written formulation (small genomes only): enumerate ALL placements of both mates on both
    strands over the whole genome, keep the concordant pairs of which at least one mate is a seed hit whose mate may
    anchor (or both are seed hits), take the top two."""
    S = Searcher(ora, g, seedl, totalkmax, scores, min_ins, max_ins)
    _, h1, o1, h2, o2 = f
    n = b1.n_reads
    out = np.zeros(n, dtype=pc.REC_DTYPE)
    N = g.sym.shape[0]
    for i in range(n):
        (r1, q1), (r2, q2) = read_of(b1, i), read_of(b2, i)
        a = (h1[int(o1[i]):int(o1[i + 1])], h2[int(o2[i]):int(o2[i + 1])])
        seeds = [{(int(x["pos"]), int(bool(x["inverted"]))) for x in a[m]} for m in range(2)]
        searchable = eligible(r1, seedl) and eligible(r2, seedl)
        may_anchor = [searchable and not (max_anchors and len(a[m]) > max_anchors) for m in range(2)]
        places = [[], []]
        for m, (rd, q) in enumerate(((r1, q1), (r2, q2))):
            if not searchable:
                for x in a[m]:
                    places[m].append((int(x["pos"]), int(bool(x["inverted"])), int(x["k"]), np.float32(x["score"]), int(x["frag"])))
                continue
            for inv in (0, 1):
                ob = oriented(rd, inv)
                if len(rd) > N:
                    continue
                k = (np.lib.stride_tricks.sliding_window_view(g.sym, len(rd)) != ob[None, :]).sum(axis=1)
                for p in np.nonzero(k <= totalkmax)[0]:
                    pl = S.placement(rd, q, inv, int(p))
                    if pl is not None:
                        places[m].append((int(p), inv, pl[0], pl[1], pl[2]))
        table = {}
        for p1, i1, k1, s1, f1 in places[0]:
            for p2, i2, k2, s2, f2 in places[1]:
                seed1, seed2 = (p1, i1) in seeds[0], (p2, i2) in seeds[1]
                if not ((seed1 and seed2) or (seed1 and may_anchor[0]) or (seed2 and may_anchor[1])):
                    continue
                if f1 != f2 or i1 == i2:
                    continue
                if i1 == 0:
                    ok = p1 <= p2 and p1 + len(r1) <= p2 + len(r2) and min_ins <= p2 + len(r2) - p1 <= max_ins
                else:
                    ok = p2 <= p1 and p2 + len(r2) <= p1 + len(r1) and min_ins <= p1 + len(r1) - p2 <= max_ins
                if ok:
                    v = float(np.float64(s1) + np.float64(s2)) if scores else -float(k1 + k2)
                    table[(fileid, f1, p1, p2, i1)] = (v, (s1, s2, k1, k2))
        out[i] = pc.record_of([(v, loc, pay) for loc, (v, pay) in table.items()], pc.eps_of(scores, filter_mult, len(r1), len(r2)))
    return out


def transitions(off, on):
    """fragments that change state when the search is switched on, counted on the checker's records"""
    so, sn = off["state"], on["state"]
    moved = np.array([pc.loc_of(a) != pc.loc_of(b) for a, b in zip(off, on)])
    return {"nomatch_unique": np.nonzero((so == pc.NOMATCH) & (sn == pc.UNIQUE))[0],
            "nomatch_nonunique": np.nonzero((so == pc.NOMATCH) & (sn == pc.NONUNIQUE))[0],
            "unique_nonunique": np.nonzero((so == pc.UNIQUE) & (sn == pc.NONUNIQUE))[0],
            "unique_better": np.nonzero((so == pc.UNIQUE) & (sn == pc.UNIQUE) & moved & (on["best"] > off["best"]))[0]}
