"""The placement stages (pileup, calls, mismatch lists, read summaries and duplicate marks) at the edges of the batch domain:
the records are the oracle's for the reads of domain_workloads.py -- 0 .. 16384 bases, quality bytes 0..127 and their 0..63
twin, reads without bases --, the expected values come from the Python checkers (test_batch_domain_cpu.py checks those
against a direct comparison at 16384 bases).  Everything is an integer and compared exactly."""
import ctypes as C
import types

import numpy as np
import pytest

import call_checker as ck
import domain_workloads as dw
import dup_checker as dk
import pairs_checker as pc
import pairs_workloads as pw
import pileup_checker as pk
import sam_checker as sk
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions

pytestmark = pytest.mark.gpu

WIDE_INS = 17_000                   # an outer distance that holds a 16384-base mate
THRESHOLDS = (0, 1)                 # min_call_qual, min_depth: every site with a best genotype other than (ref, ref) is a call
CALL_COUNTS = ck.COUNTERS + ("calls", "het", "hom")
PILEUP_COUNTS = pk.COUNTERS + ("covered", "sites", "max_depth")


@pytest.fixture(scope="module")
def matcher():
    """the workload's text without an index: no stage needs one"""
    import torch
    torch.zeros(1, device="cuda")      # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    w = dw.workload()
    m = PairMatcher(RealOptions(seedl=32, seedkmax=dw.SEEDKMAX, totalkmax=dw.TOTALKMAX, scores=True).normalise())
    m.set_text_symbols(0, w.g.sym, w.g.frag_start)
    yield m
    m.close()


def _equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for k in want.dtype.names:
        if k != "reserved":
            assert np.array_equal(got[k], want[k]), (what, k, np.nonzero((got[k] != want[k]).reshape(got.shape[0], -1).any(axis=1))[0][:10])


def _same_lists(got, want, what):
    (gl, go), (wl, wo, _) = got, want
    assert np.array_equal(go, wo), (what, np.nonzero(go != wo)[0][:10])
    assert gl.shape == wl.shape, (what, gl.shape, wl.shape)
    for k in ("off", "ref", "base"):
        assert np.array_equal(gl[k], wl[k]), (what, k, np.nonzero(gl[k] != wl[k])[0][:10])


def _pileup_and_calls(m, sym, min_qual, add, call_add, want_add, what):
    """pileup and calls of one add against the checkers -> (checker pileup, checker calls)"""
    pu = pk.Pileup(sym, 0, min_qual)
    want_add(pu)
    cl = ck.Calls(pu)
    want_add(cl)
    m.pileup_stats(reset=True)
    m.call_stats(reset=True)
    m.pileup_begin(min_qual)
    add()
    assert m.pileup_finish() == pu.sites().shape[0], what
    _equal(m.pileup_sites(), pu.sites(), (what, "sites"))
    assert np.array_equal(m.pileup_depth(0, pu.n).astype(np.int64), pu.depth), (what, "depth")
    st, wst = m.pileup_stats(), pu.finish_stats()
    assert {k: st[k] for k in PILEUP_COUNTS} == wst, (what, st, wst)
    m.call_begin()
    call_add()
    want = cl.calls(*THRESHOLDS)
    assert m.call_finish(*THRESHOLDS) == want.shape[0], what
    _equal(m.call_evidence(), cl.evidence(), (what, "evidence"))
    _equal(m.call_variants(), want, (what, "calls"))
    st, wst = m.call_stats(), cl.finish_stats(*THRESHOLDS)
    assert {k: st[k] for k in CALL_COUNTS} == wst, (what, st, wst)
    m.call_end()
    m.pileup_end()
    return pu, cl


def _single_stages(m, sym, b, info, min_qual, what):
    """every single-end stage on batch b with the records info, against the checkers"""
    pu, _ = _pileup_and_calls(m, sym, min_qual, lambda: m.pileup_add(b.bases, b.qual, info, offsets=b.offsets),
                              lambda: m.call_add(b.bases, b.qual, info, offsets=b.offsets), lambda x: x.add(b, info), what)
    want = sk.mismatch_lists(sym, 0, sk.final_single(info), sk.single_reads(b))
    m.mismatch_stats(reset=True)
    _same_lists(m.mismatches(b.bases, None, info, offsets=b.offsets, cap=want[0].shape[0] + 1), want, what)   # (room for all: one call)
    st = m.mismatch_stats()
    assert {k: st[k] for k in sk.COUNTERS} == want[2], (what, st, want[2])
    sums = m.read_summary(b.bases, b.qual, b.offsets, min_qual=min_qual)
    wsums = dk.summaries_of(b, min_qual)
    assert np.array_equal(sums["len"], wsums["len"]) and np.array_equal(sums["qsum"], wsums["qsum"]), what
    m.dup_stats(reset=True)
    dup = m.mark_duplicates(info, sums)
    wdup, wst, _ = dk.mark_single(info, wsums)
    assert np.array_equal(dup, wdup), (what, np.nonzero(dup != wdup)[0][:10])
    st = m.dup_stats()
    assert {k: st[k] for k in dk.STATS} == wst, (what, st, wst)
    return pu, want, wsums, wst


@pytest.mark.parametrize("min_qual", [0, 20, 63])
@pytest.mark.parametrize("which", ["b", "b63"])
def test_single_end_stages_on_the_oracles_records(ora, matcher, which, min_qual):
    w = dw.workload()
    b = dw.batch_of(w, which)
    info = dw.oracle(ora, which, 32, 1).info
    pu, lists, sums, dst = _single_stages(matcher, w.g.sym, b, info, min_qual, (which, min_qual))
    lens = dw.lens_of(b)
    assert pu.stats["placed"] > 200 and pu.stats["invalid"] == 0 and pu.finish_stats()["max_depth"] >= 2
    assert lists[2]["disagree"] == 0 and lists[2]["mismatches"] >= 9 * dw.TOTALKMAX
    assert int(lists[0]["off"].max()) == 16383
    if min_qual == 0:                       # a qsum no read of qualities below 64 reaches, and beyond what the marks tell apart
        assert (int(sums["qsum"].max()) > (1 << 20) - 1) == (which == "b") and (which == "b" or int(sums["qsum"].max()) <= 16384 * 63)
    assert dst["duplicates"] >= 1           # (reads of several lengths start at one position)
    if min_qual:
        assert pu.stats["low_qual"] > 0
    assert (lens == 16384).sum() == 13


@pytest.mark.parametrize("min_qual", [0, 20, 63])
@pytest.mark.parametrize("which", ["b", "b63"])
def test_paired_stages_on_the_checkers_records(ora, matcher, which, min_qual):
    """mates of (2049, 100), (100, 16384), (0, 100) and (100, 31) bases, the pair records from pairs_checker on the oracle's lists"""
    m = matcher
    w = dw.workload()
    b1, b2 = w.pairs if which == "b" else (dw.twin(w.pairs[0]), dw.twin(w.pairs[1]))
    o1, o2 = dw.oracle(ora, "pairs1", 32, 1), dw.oracle(ora, "pairs2", 32, 1)
    pairs = pc.check_pairs([(0, o1.hits, o1.hoff, o2.hits, o2.hoff)], pw.lens_of(b1), pw.lens_of(b2), pw.MIN_INS, WIDE_INS, 1,
                           ora.filter_mult(2, dw.TOTALKMAX)).astype(rlib.PAIR_DTYPE)
    assert (pairs["state"] == pc.UNIQUE).sum() == 6 and set(pairs["inverted1"][pairs["state"] == pc.UNIQUE]) == {0, 1}
    what = ("pairs", which, min_qual)
    pu, _ = _pileup_and_calls(m, w.g.sym, min_qual, lambda: m.pileup_add_pairs(b1, b2, pairs), lambda: m.call_add_pairs(b1, b2, pairs),
                              lambda x: x.add_pairs(b1, b2, pairs), what)
    assert pu.stats["placed"] == 12 and pu.stats["bases"] == 3 * (2049 + 100) + 3 * (100 + 16384)
    assert pu.stats["mismatches"] + pu.stats["low_qual"] == 12
    want = sk.mismatch_lists(w.g.sym, 0, sk.final_pairs(pairs), sk.pair_reads(b1, b2))
    m.mismatch_stats(reset=True)
    _same_lists(m.mismatches_pairs(b1, b2, pairs), want, what)
    st = m.mismatch_stats()
    assert {k: st[k] for k in sk.COUNTERS} == want[2], (what, st, want[2])
    s1, s2 = (m.read_summary(b.bases, b.qual, b.offsets, min_qual=min_qual) for b in (b1, b2))
    w1, w2 = dk.summaries_of(b1, min_qual), dk.summaries_of(b2, min_qual)
    for got, ws in ((s1, w1), (s2, w2)):
        assert np.array_equal(got["len"], ws["len"]) and np.array_equal(got["qsum"], ws["qsum"]), what
    m.dup_stats(reset=True)
    dup = m.mark_duplicates_pairs(pairs, s1, s2)
    wdup, wst, _ = dk.mark_pairs(pairs, w1, w2)
    assert np.array_equal(dup, wdup) and {k: m.dup_stats()[k] for k in dk.STATS} == wst, (what, dup, wdup)


@pytest.mark.parametrize("which", ["empty", "edge_empty"])
def test_every_stage_on_reads_without_bases(ora, matcher, which):
    w = dw.workload()
    b = dw.batch_of(w, which)
    info = dw.oracle(ora, which, 32, 1).info
    pu, lists, sums, dst = _single_stages(matcher, w.g.sym, b, info, 20, which)
    assert sums["len"][0] == 0 and sums["qsum"][0] == 0 and lists[1][1] == 0
    if which == "empty":
        assert pu.stats["placed"] == 0 and pu.stats["reads"] == 5 and dst["placed"] == 0 and lists[0].shape[0] == 0
        # records that claim a placement for a read without bases (no matcher writes them): a placement of no bases, counted as
        # placed; one 5' end for all five, so four of them are duplicates
        claimed = np.full(5, (1 << 61) | 1000, dtype=np.uint64)
        _single_stages(matcher, w.g.sym, b, claimed, 0, "claimed")
    else:
        assert pu.stats["placed"] >= 10
    # pairs of mates without bases
    none = types.SimpleNamespace(bases=w.empty.bases, qual=w.empty.qual, offsets=w.empty.offsets)
    pairs = np.zeros(5, dtype=rlib.PAIR_DTYPE)
    _pileup_and_calls(matcher, w.g.sym, 0, lambda: matcher.pileup_add_pairs(none, none, pairs), lambda: matcher.call_add_pairs(none, none, pairs),
                      lambda x: x.add_pairs(none, none, pairs), "empty pairs")


# ---- hand-made records -------------------------------------------------------------------------------------------------
def _info(state, pos):
    return np.uint64((state << 61) | pos)


def _hand(reads):
    """[(bases, qual)] -> a batch object"""
    return types.SimpleNamespace(bases=np.concatenate([r[0] for r in reads]).astype(np.uint8), qual=np.concatenate([r[1] for r in reads]).astype(np.uint8),
                                 offsets=np.cumsum([0] + [r[0].shape[0] for r in reads]).astype(np.uint64), n_reads=len(reads))


def test_a_long_read_on_unrelated_text_and_the_overflow_protocol(matcher):
    """16384 random bases placed mid-text on both strands: about three quarters of the offsets are in the list, the last one is
    16383; a buffer one entry short is REAL_HIP_E_OVERFLOW with the count and nothing written"""
    m = matcher
    w = dw.workload()
    rng = np.random.default_rng(41)
    reads = []
    for inv in (0, 1):
        r = rng.integers(0, 4, size=16384).astype(np.uint8)
        o = synth.revcomp(r) if inv else r
        for j in (0, 16383):                                    # the oriented read differs from the text at both ends
            o[j] = (w.g.sym[30_000 + j] + 1) & 3
        reads.append((synth.revcomp(o) if inv else o, rng.integers(0, 128, size=16384).astype(np.uint8)))
    b = _hand(reads)
    info = np.array([_info(1, 30_000), _info(2, 30_000)], dtype=np.uint64)
    _, want, _, dst = _single_stages(m, w.g.sym, b, info, 20, "unrelated")
    wl, wo, wst = want
    total = wl.shape[0]
    assert 2 * 12_000 < total < 2 * 12_600 and wl["off"][int(wo[1]) - 1] == 16383 and wl["off"][-1] == 16383 and wl["off"][0] == 0
    assert dst["duplicates"] == 0                               # (the two strands' 5' ends differ)
    batch = m._read_batch(b.bases, None, b.offsets, host_records=True)
    out = np.full(total + 1, 0x07070707, dtype=np.uint32)
    off = np.zeros(3, dtype=np.uint64)
    nout = C.c_uint64(0)
    call = m._L.real_hip_mismatches
    assert call(m._h, C.byref(batch), info.ctypes.data, out.ctypes.data, total - 1, C.byref(nout), off.ctypes.data) == rlib.REAL_HIP_E_OVERFLOW
    assert nout.value == total and (out == 0x07070707).all(), "nothing is written on overflow"
    assert call(m._h, C.byref(batch), info.ctypes.data, out.ctypes.data, total, C.byref(nout), off.ctypes.data) == rlib.REAL_HIP_OK
    assert nout.value == total and out[-1] == 0x07070707 and np.array_equal(off, wo)
    assert np.array_equal(out[:-1].view(rlib.MISMATCH_DTYPE)["off"], wl["off"])
    _same_lists(m.mismatches(b.bases, None, info, offsets=b.offsets, cap=1), want, "the mirror grows its buffer once")


def test_a_long_placement_that_ends_on_the_last_base_and_one_behind_it(matcher):
    m = matcher
    w = dw.workload()
    n = w.g.n
    rng = np.random.default_rng(42)
    reads = []
    for inv in (0, 1, 0, 1):
        o = w.g.sym[n - 16384:n].copy()
        o[::1000] = (o[::1000] + 1) & 3
        o[16383] = (o[16383] + 2) & 3
        reads.append((synth.revcomp(o) if inv else o, rng.integers(0, 128, size=16384).astype(np.uint8)))
    b = _hand(reads)
    info = np.array([_info(1, n - 16384), _info(2, n - 16384), _info(1, n - 16383), _info(2, n - 16383)], dtype=np.uint64)
    for min_qual in (0, 63):
        pu, want, _, _ = _single_stages(m, w.g.sym, b, info, min_qual, ("the end", min_qual))
        assert pu.stats["placed"] == 2 and pu.stats["invalid"] == 2 and pu.depth[n - 1] == 2 and want[2]["invalid"] == 2
        assert want[0]["off"][int(want[1][1]) - 1] == 16383 and want[1][4] == want[1][2]


def test_summaries_of_quality_127_and_the_clamp_of_the_marks(matcher):
    """16384 x 127 = 2080768 is what the summary holds; the marks count it as 2^20 - 1"""
    m = matcher
    top = (1 << 20) - 1
    rng = np.random.default_rng(43)
    reads = [(rng.integers(0, 4, size=L).astype(np.uint8), np.full(L, 127, np.uint8)) for L in (16384, 16384, 8257, 16383)]
    b = _hand(reads)
    for min_qual in (0, 63):
        sums = m.read_summary(b.bases, b.qual, b.offsets, min_qual=min_qual)
        assert sums["qsum"].tolist() == [2080768, 2080768, 8257 * 127, 16383 * 127] and sums["len"].tolist() == [16384, 16384, 8257, 16383]
    assert 8257 * 127 > top > 8256 * 127
    hand = np.zeros(6, dtype=rlib.READ_SUM_DTYPE)
    hand["len"] = 100
    # one position, one strand: 2^20 - 1 against 2^20 + 5 is a tie (the smaller index stays), 2^20 - 2 loses; then the summaries above
    hand["qsum"] = (top, top + 6, top - 1, top + 6, 2080768, top)
    info = np.array([_info(1, 500), _info(1, 500), _info(1, 900), _info(1, 900), _info(2, 700), _info(2, 700)], dtype=np.uint64)
    dup = m.mark_duplicates(info, hand)
    wdup, wst, _ = dk.mark_single(info, hand)
    assert wdup.tolist() == [0, 1, 1, 0, 0, 1] and np.array_equal(dup, wdup), (dup, wdup)
    info4 = np.array([_info(1, 500)] * 4, dtype=np.uint64)
    dup = m.mark_duplicates(info4, sums)                         # 2080768, 2080768, 1048639, 2080641: all count as 2^20 - 1
    assert dup.tolist() == [0, 1, 1, 1] and np.array_equal(dup, dk.mark_single(info4, sums)[0])
    # pairs: each mate's qsum is clamped, then the two are added
    pairs = np.zeros(3, dtype=rlib.PAIR_DTYPE)
    pairs["state"], pairs["pos1"], pairs["pos2"] = pc.UNIQUE, 100, 300
    s1, s2 = np.zeros(3, dtype=rlib.READ_SUM_DTYPE), np.zeros(3, dtype=rlib.READ_SUM_DTYPE)
    s1["len"], s2["len"] = 100, 100
    s1["qsum"], s2["qsum"] = (top, 1, 2080768), (0, 2080768, 5)
    dup = m.mark_duplicates_pairs(pairs, s1, s2)
    wdup = dk.mark_pairs(pairs, s1, s2)[0]
    assert wdup.tolist() == [1, 1, 0] and np.array_equal(dup, wdup), (dup, wdup)   # 2^20 - 1, 2^20, 2^20 + 4
