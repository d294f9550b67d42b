"""What domain_workloads.py claims, shown with the oracle alone (no GPU): every length of LENS is placed on both strands at a
fragment's first base, on the text's last base and mid-text, reaches totalkmax and passes it, meets the exact and the near
copy; quality bytes beyond 63 change the score bits, and a `+` in the table index is not the reference's `|`.  Then the
Python checkers of the placement stages against a direct numpy comparison of read and text at 16384 bases, and the clamp of
dup_checker.mark."""
import numpy as np

import call_checker as ck
import domain_workloads as dw
import dup_checker as dk
import pileup_checker as pk
import sam_checker as sk
from real_amd import synth

PLACED_LENS = [L for L in dw.LENS if L >= 32]
NONUNIQUE = 4                       # UniqueMatchInfo.hpp:29-39: NoMatch 0, Straight 1, Reverse 2, Gapped 3, NonUnique 4


def _state(info):
    return (np.asarray(info, dtype=np.uint64) >> np.uint64(61)).astype(np.int64)


def _pos(info):
    return (np.asarray(info, dtype=np.uint64) & np.uint64((1 << 35) - 1)).astype(np.int64)


def _errors(info):
    return ((np.asarray(info, dtype=np.uint64) >> np.uint64(41)) & np.uint64(15)).astype(np.int64)


def _read(b, i):
    return b.bases[int(b.offsets[i]):int(b.offsets[i + 1])], b.qual[int(b.offsets[i]):int(b.offsets[i + 1])]


def test_the_workload_is_what_the_issue_describes():
    w = dw.workload()
    g, b = w.g, w.b
    assert g.n == 200_000 and g.n_frag == 2 and len(dw.N_RUNS) == 2 and all((g.sym[lo:hi] == 4).all() for lo, hi in dw.N_RUNS)
    assert dw.COPY_LEN >= 16400
    assert np.array_equal(g.sym[dw.EXACT_SRC:dw.EXACT_SRC + dw.COPY_LEN], g.sym[dw.EXACT_DST:dw.EXACT_DST + dw.COPY_LEN])
    differ = np.nonzero(g.sym[dw.NEAR_SRC:dw.NEAR_SRC + dw.COPY_LEN] != g.sym[dw.NEAR_DST:dw.NEAR_DST + dw.COPY_LEN])[0]
    assert np.array_equal(differ, np.arange(dw.NEAR_FIRST, dw.COPY_LEN, dw.NEAR_EVERY))           # two per 2000 bases
    lens = dw.lens_of(b)
    assert set(lens.tolist()) == set(dw.LENS) | {dw.FILL_LEN} and int((lens == dw.FILL_LEN).sum()) == dw.N_FILL
    assert b.n_reads < 450 and int(b.qual.max()) == 127 and int(w.b63.qual.max()) == 63
    assert np.array_equal(w.b63.qual, b.qual & 63) and w.b63.bases is b.bases
    for i in range(b.n_reads):                                  # 63, 64, 93 and 127 in the first and in the last 16 bases
        q = _read(b, i)[1]
        if q.shape[0] >= 16:
            assert set(dw.FORCED_Q) <= set(q[:16].tolist()) and set(dw.FORCED_Q) <= set(q[-16:].tolist()), i
    # long reads sit next to short ones: every wave's 64 reads hold reads over 320 bases and 100-base reads
    for lo in range(0, b.n_reads, 64):
        tile = lens[lo:lo + 64]
        assert (tile > 320).any() and (tile == dw.FILL_LEN).any(), lo
    for L in dw.UNIFORM:
        u = w.uniform[L]
        assert u.n_reads == 13 and (dw.lens_of(u) == L).all()
    assert w.empty.n_reads == 5 and w.empty.bases.shape[0] == 0 and int(w.empty.offsets[-1]) == 0
    el = dw.lens_of(w.edge_empty)
    assert el[0] == 0 and el[-1] == 0 and (el[1:-1] > 0).all() and el.shape[0] == 22
    got = sorted(set(zip(dw.lens_of(w.pairs[0]).tolist(), dw.lens_of(w.pairs[1]).tolist())))
    assert got == sorted(set(dw.PAIR_LENS))
    for L in PLACED_LENS:                                       # the substitutions of the read with totalkmax errors
        at = dw.subst_offsets(L, dw.TOTALKMAX)
        assert len(at) == dw.TOTALKMAX and at[0] == 0 and at[-1] == L - 1
        assert L <= 2048 or 2047 in at or 2048 in at
        assert len(dw.subst_offsets(L, dw.TOTALKMAX + 1)) == dw.TOTALKMAX + 1


def _by(w, L, kind, inv=0):
    return dw.index_of(w, L, kind, inv)


def test_every_length_is_placed_on_both_strands_at_the_three_positions(ora):
    w = dw.workload()
    for scores in (1, 0):
        o = dw.oracle(ora, "b", 32, scores)
        st, pos = _state(o.info), _pos(o.info)
        for L in PLACED_LENS:
            for kind in ("first", "end", "mid"):
                for inv in (0, 1):
                    i = _by(w, L, kind, inv)
                    assert st[i] == 1 + inv and pos[i] == w.meta[i][3] and _errors(o.info)[i] == 0, (scores, L, kind, inv, st[i], pos[i])
                    assert o.hoff[i + 1] - o.hoff[i] == 1
            assert pos[_by(w, L, "end")] + L == w.g.n and pos[_by(w, L, "first")] == int(w.g.frag_start[1])


def test_every_length_reaches_totalkmax_and_passes_it(ora):
    """with 32-base seeds a 32-base read is its own seed and holds at most seedkmax = 2 errors: that length reaches totalkmax = 3
    with the 16-base seeds of the bucket-row geometry only"""
    w = dw.workload()
    for seedl, lens in ((32, [L for L in PLACED_LENS if L > 32]), (16, PLACED_LENS)):
        for scores in (1, 0):
            o = dw.oracle(ora, "b", seedl, scores)
            st = _state(o.info)
            for L in lens:
                i, j = _by(w, L, "kmax"), _by(w, L, "over")
                assert st[i] == 1 and _errors(o.info)[i] == dw.TOTALKMAX and _pos(o.info)[i] == dw.P_KMAX, (seedl, scores, L, st[i])
                assert st[j] == 0 and o.hoff[j + 1] == o.hoff[j], (seedl, scores, L, st[j])


def test_the_copies_give_nonunique_and_the_better_side(ora):
    """the exact copy: two locations of equal value, NonUnique whatever decides.  The near copy: with scores off the error count
    decides and the read is Unique on its source for every length; with scores on and eps = filter_mult * L a copy with one
    or two more mismatches stays inside eps (NonUnique: the record is still compared bit for bit) until the copy has more than
    totalkmax errors, from 4096 bases on"""
    w = dw.workload()
    for scores in (1, 0):
        o = dw.oracle(ora, "b", 32, scores)
        st, pos = _state(o.info), _pos(o.info)
        for L in PLACED_LENS:
            for inv in (0, 1):
                i = _by(w, L, "exact", inv)
                assert st[i] == NONUNIQUE and o.hoff[i + 1] - o.hoff[i] == 2, (scores, L, inv, st[i])
                i = _by(w, L, "near", inv)
                n_other = int(o.hoff[i + 1] - o.hoff[i]) - 1
                assert n_other == (1 if L <= 2049 else 0), (L, n_other)
                if not scores or L >= 4096:
                    assert st[i] == 1 + inv and pos[i] == dw.P_NEAR and _errors(o.info)[i] == 0, (scores, L, inv, st[i])


def test_short_empty_and_n_reads_are_nomatch_without_hits(ora):
    w = dw.workload()
    for scores in (1, 0):
        o = dw.oracle(ora, "b", 32, scores)
        st = _state(o.info)
        seen = 0
        for i, m in enumerate(w.meta):
            if m[0] in (0, 31) or m[1] == "n":
                assert st[i] == 0 and o.info[i] == 0 and o.hoff[i + 1] == o.hoff[i], (i, m)
                seen += 1
        assert seen == 3 + 13 + len(dw.LENS) - 2
    for which in ("empty", "edge_empty"):
        o = dw.oracle(ora, which)
        b = dw.batch_of(w, which)
        assert o.info.shape[0] == b.n_reads and o.info[0] == 0 and o.info[-1] == 0 and o.hoff[1] == 0
    assert not dw.oracle(ora, "empty").info.any() and dw.oracle(ora, "empty").hits.shape[0] == 0
    assert (_state(dw.oracle(ora, "edge_empty").info) != 0).sum() >= 10


# ---- quality bytes beyond 63 ---------------------------------------------------------------------------------------------
def _numpy_score(LL, text, read, qual, p, inverted, index):
    """ComputeScore.hpp:50-190 in numpy: 1.0 plus the table entries in base order, summed one after the other in FP64 (cumsum
    adds in order), cast to float once; index(ref, base, q) says how the three meet"""
    L = read.shape[0]
    o = (3 - read[::-1].astype(np.int64)) if inverted else read.astype(np.int64)
    q = (qual[::-1] if inverted else qual).astype(np.int64)
    ref = text[p:p + L].astype(np.int64)
    terms = np.concatenate([[1.0], LL[index(ref, o, q) & 1023]])
    return np.float32(np.cumsum(terms)[-1])


def test_quality_bytes_beyond_63_reach_the_read_base_bits(ora):
    w = dw.workload()
    o, o63 = dw.oracle(ora, "b", 32, 1), dw.oracle(ora, "b63", 32, 1)
    LL, _ = ora.scoring_table()
    text = np.where(w.g.sym > 3, 0, w.g.sym)
    st = _state(o.info)
    placed = np.nonzero((st == 1) | (st == 2))[0]
    assert placed.shape[0] > 200
    bits, bits63 = o.score.view(np.uint32), o63.score.view(np.uint32)
    same_place = placed[(o.info[placed] == o63.info[placed])]
    assert (bits[same_place] != bits63[same_place]).mean() >= 0.9 and same_place.shape[0] >= 0.9 * placed.shape[0]
    assert (bits[placed] != bits63[placed]).mean() >= 0.9
    plus_differs = {}
    for i in placed:
        L = w.meta[i][0]
        r, q = _read(w.b, i)
        args = (LL, text, r, q, int(_pos(o.info)[i]), st[i] == 2)
        s_or = _numpy_score(*args, lambda ref, rb, qq: (ref << 8) | (rb << 6) | qq)
        assert s_or.view(np.uint32) == bits[i], (i, w.meta[i], s_or, o.score[i])              # the restatement is the oracle's
        s_plus = _numpy_score(*args, lambda ref, rb, qq: (ref << 8) + (rb << 6) + qq)
        plus_differs[L] = plus_differs.get(L, 0) + int(s_plus.view(np.uint32) != bits[i])
        s_and = _numpy_score(*args, lambda ref, rb, qq: (ref << 8) | (rb << 6) | (qq & 63))
        assert s_and.view(np.uint32) == bits63[i] or o.info[i] != o63.info[i]
    assert set(plus_differs) == set(PLACED_LENS) | {dw.FILL_LEN}
    assert all(v >= 1 for v in plus_differs.values()), plus_differs


# ---- the stage checkers at 16384 bases -----------------------------------------------------------------------------------
def _long_placements(ora):
    """the 16384-base reads the oracle places, on both strands: (read index, position, inverted)"""
    w = dw.workload()
    o = dw.oracle(ora, "b", 32, 1)
    st = _state(o.info)
    out = [(i, int(_pos(o.info)[i]), st[i] == 2) for i, m in enumerate(w.meta) if m[0] == 16384 and st[i] in (1, 2)]
    assert {inv for _, _, inv in out} == {False, True} and len(out) >= 7
    return w, o, out


def _direct(w, i, p, inv):
    """oriented read, oriented qualities, text symbols under it, compared base by base"""
    r, q = _read(w.b, i)
    o = synth.revcomp(r) if inv else r
    oq = q[::-1] if inv else q
    t = w.g.sym[p:p + r.shape[0]]
    return o, oq, t, np.nonzero(o != t)[0]


def test_the_stage_checkers_at_16384_bases_against_a_direct_comparison(ora):
    w, o, places = _long_placements(ora)
    n = w.g.n
    for min_qual in (0, 20, 63):
        depth = np.zeros(n, np.int64)
        alt = np.zeros((n, 4), np.int64)
        low = mism = 0
        pu = pk.Pileup(w.g.sym, 0, min_qual)
        for i, p, inv in places:
            ob, oq, t, at = _direct(w, i, p, inv)
            assert (t <= 3).all()
            depth[p:p + 16384] += 1
            for j in at:
                if oq[j] < min_qual:
                    low += 1
                else:
                    mism += 1
                    alt[p + j, ob[j]] += 1
            pu.place(*_read(w.b, i), p, inv)
        assert np.array_equal(pu.depth, depth) and np.array_equal(pu.alt, alt)
        assert pu.stats["low_qual"] == low and pu.stats["mismatches"] == mism and pu.stats["bases"] == 16384 * len(places)
        assert mism + low >= dw.TOTALKMAX
        # the calls' evidence on the pileup's sites: counts and quality sums of every base seen there, by hand
        cl = ck.Calls(pu)
        for i, p, inv in places:
            cl.place(*_read(w.b, i), p, inv)
        sites = pu.sites()["pos"].astype(np.int64)
        cnt = np.zeros((sites.shape[0], 4), np.int64)
        for i, p, inv in places:
            ob, oq, t, _ = _direct(w, i, p, inv)
            for s, x in enumerate(sites):
                if p <= x < p + 16384 and oq[x - p] >= min_qual:
                    cnt[s, ob[x - p]] += 1
        ev = cl.evidence()
        assert np.array_equal(ev["cnt"].astype(np.int64), cnt), min_qual
    # the mismatch lists: offsets up to 16383, text and oriented base
    fin = sk.final_single(o.info)
    lists, off, st = sk.mismatch_lists(w.g.sym, 0, fin, sk.single_reads(w.b))
    assert st["disagree"] == 0 and st["on_n"] == 0
    last = 0
    for i, p, inv in places:
        ob, _, t, at = _direct(w, i, p, inv)
        L = lists[int(off[i]):int(off[i + 1])]
        assert np.array_equal(L["off"], at) and np.array_equal(L["ref"], t[at]) and np.array_equal(L["base"], ob[at])
        assert L.shape[0] == int(_errors(o.info)[i])
        last = max(last, int(at.max()) if at.size else 0)
    assert last == 16383
    # the summaries and the 5' ends of the duplicate keys
    for min_qual in (0, 20, 63):
        sums = dk.summaries_of(w.b, min_qual)
        keys = dk.keys_single(o.info, sums)
        for i, p, inv in places:
            q = _read(w.b, i)[1].astype(np.int64)
            assert sums["len"][i] == 16384 and sums["qsum"][i] == int(q[q >= min_qual].sum())
            assert keys[i] == (0, 2 if inv else 1, p + 16383 if inv else p)
    assert int(dk.summaries_of(w.b, 0)["qsum"].max()) > 16384 * 63 and int(dk.summaries_of(w.b63, 0)["qsum"].max()) < 1 << 20


def test_the_clamp_of_the_duplicate_quality():
    """include/real_hip.h: "a qsum beyond 2^20 - 1 counts as 2^20 - 1" (per mate for pairs)"""
    top = (1 << 20) - 1
    key = (0, 1, 1000)
    dup, st, _ = dk.mark([key, key], np.array([top, top + 6]))
    assert dup.tolist() == [0, 1] and st["duplicates"] == 1                   # a tie: the smaller index stays
    dup, _, _ = dk.mark([key, key], np.array([top + 6, top]))
    assert dup.tolist() == [0, 1]
    dup, _, _ = dk.mark([key, key], np.array([top - 1, top + 6]))
    assert dup.tolist() == [1, 0]                                             # 2^20 - 2 loses
    info = np.array([(1 << 61) | 1000, (1 << 61) | 1000], dtype=np.uint64)
    sums = np.zeros(2, dtype=dk.SUM_DTYPE)
    sums["len"], sums["qsum"] = 16384, (top, 16384 * 127)
    assert dk.mark_single(info, sums)[0].tolist() == [0, 1]
    # pairs: each mate's qsum is clamped, then the two are added
    pairs = np.zeros(2, dtype=[("state", "u1"), ("inverted1", "u1"), ("pos1", "<u4"), ("pos2", "<u4"), ("fileid", "u1")])
    pairs["state"], pairs["pos1"], pairs["pos2"] = dk.UNIQUE, 100, 300
    s1, s2 = np.zeros(2, dtype=dk.SUM_DTYPE), np.zeros(2, dtype=dk.SUM_DTYPE)
    s1["len"], s2["len"] = 100, 100
    s1["qsum"], s2["qsum"] = (top, top + 500), (10, 10)
    assert dk.mark_pairs(pairs, s1, s2)[0].tolist() == [0, 1]                 # a tie after the clamp
    s1["qsum"], s2["qsum"] = (top + 500, 0), (0, top + 400)
    assert dk.mark_pairs(pairs, s1, s2)[0].tolist() == [0, 1]                 # per mate: 2^20 - 1 + 0 on both sides
    s2["qsum"] = (0, top + 1 + top)                                           # (the sum alone, clamped once, would win here too)
    s1["qsum"] = (top, 1)
    assert dk.mark_pairs(pairs, s1, s2)[0].tolist() == [1, 0]                 # 2^20 - 1 + 0 against 1 + 2^20 - 1
