"""Duplicate marking on the device (real_hip_read_summary, real_hip_mark_duplicates, real_hip_mark_duplicates_pairs) against
dup_checker.py, which restates it in numpy / pure Python.  The records of the workloads come from match_unique / match_pairs on
the device and are first asserted to be the oracle's / the pair checker's.  Everything is an integer and compared exactly."""
import ctypes as C
import types

import numpy as np
import pytest

import dup_checker as dk
import dup_workloads as dw
import insert_workloads as iw
import pairs_checker as pc
import pileup_workloads as pw
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions, UniqueMatcher

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def single(ora):
    """a matcher with the single-end workload's text and index, and the device-matched records of both batches, asserted to be
    the oracle's"""
    import torch
    torch.zeros(1, device="cuda")      # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    dw.assert_single_conditions(ora)
    w = pw.workload()
    m = UniqueMatcher(RealOptions(seedl=pw.SEEDL, seedkmax=pw.SEEDK, totalkmax=pw.TOTALK, scores=True, filter_level=pw.FILTER_LEVEL).normalise())
    m.set_text_symbols(0, w.g.sym, w.g.frag_start)
    m.build_index_block()
    rec = {}
    for which in ("main", "long"):
        b = getattr(w, which)
        info, _ = m.match_unique(b.bases, b.qual, offsets=b.offsets)
        assert np.array_equal(info, pw.oracle_records(ora, which, 1)[0]), which
        rec[which] = info
    yield m, rec
    m.close()


@pytest.fixture(scope="module")
def bare():
    """a context without text or index: the marking and the summaries need neither"""
    import torch
    torch.zeros(1, device="cuda")
    m = UniqueMatcher(RealOptions(seedl=32, seedkmax=2, totalkmax=3, scores=True, filter_level=2).normalise())
    yield m
    m.close()


def _dev(a):
    import torch
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_sums(s):
    return _dev(s.view(np.int32).reshape(-1, 2))


def _slice(b, lo, hi):
    a, e = int(b.offsets[lo]), int(b.offsets[hi])
    return types.SimpleNamespace(bases=b.bases[a:e], qual=None if b.qual is None else b.qual[a:e],
                                 offsets=(b.offsets[lo:hi + 1] - b.offsets[lo]).astype(np.uint64))


def _summary(m, b, min_qual, on_device=0, packed=False, shift=0):
    """read_summary of the batch in the form asked for -> numpy records.  shift: the device qualities start `shift` bytes behind
    an aligned address"""
    bases, nflags = (synth.pack_bases(b.bases), synth.read_nflags(b.bases, b.offsets)) if packed else (b.bases, None)
    qual, off = b.qual, b.offsets
    if not on_device:
        return m.read_summary(bases, qual, offsets=off, packed=packed, nflags=nflags, min_qual=min_qual)
    import torch
    if qual is not None:
        room = torch.zeros(qual.shape[0] + shift + 8, dtype=torch.uint8, device="cuda")
        room[shift:shift + qual.shape[0]] = _dev(qual)
        qual = room[shift:shift + qual.shape[0]]
        assert qual.data_ptr() % 4 == shift % 4
    bases, off = _dev(bases), _dev(off)
    nflags = None if nflags is None else _dev(nflags)
    if on_device == 2:
        return m.read_summary(bases, qual, offsets=off, packed=packed, nflags=nflags, min_qual=min_qual, out=np.zeros(off.shape[0] - 1, dtype=rlib.READ_SUM_DTYPE))
    out = m.read_summary(bases, qual, offsets=off, packed=packed, nflags=nflags, min_qual=min_qual)
    return out.cpu().numpy().view(np.uint32).reshape(-1, 2).copy().view(rlib.READ_SUM_DTYPE).reshape(-1)


def _same_sums(got, want, what):
    assert got.dtype == rlib.READ_SUM_DTYPE and got.shape == want.shape, what
    for k in ("len", "qsum"):
        assert np.array_equal(got[k], want[k]), (what, k, np.nonzero(got[k] != want[k])[0][:10])


# ---- summaries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_reads", [1, 63, 65, 257, 2014])
@pytest.mark.parametrize("on_device", [0, 1, 2])
def test_summaries_of_ragged_batches(bare, n_reads, on_device):
    b = _slice(pw.workload().main, 0, n_reads)
    for min_qual in (0, 15, 63):
        _same_sums(_summary(bare, b, min_qual, on_device, shift=n_reads % 4), dk.summaries_of(b, min_qual), (n_reads, on_device, min_qual))
    st = bare.dup_stats(reset=True)
    assert st["launches"] == 3 and st["kernel_ms"] > 0 and st["reads"] == st["placed"] == 0


def _short_and_unaligned():
    """reads of 1..12 bases and a few long ones, concatenated: every (start address mod 4, length mod 4) occurs"""
    rng = np.random.default_rng(3)
    lens = [1, 2, 3, 4, 5, 6, 7, 8] + [int(x) for x in rng.integers(1, 13, size=200)] + [321, 33, 322, 34, 323, 35, 700, 320]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    b = types.SimpleNamespace(bases=rng.integers(0, 4, size=int(off[-1])).astype(np.uint8), qual=rng.integers(0, 64, size=int(off[-1])).astype(np.uint8), offsets=off)
    assert {(int(o) % 4, L % 4) for o, L in zip(off[:-1], lens)} == {(a, c) for a in range(4) for c in range(4)}
    return b


@pytest.mark.parametrize("on_device,shift", [(0, 0), (1, 0), (1, 1), (1, 2), (2, 3)])
def test_summaries_of_short_reads_at_every_byte_address(bare, on_device, shift):
    b = _short_and_unaligned()
    for min_qual in (0, 15, 63):
        _same_sums(_summary(bare, b, min_qual, on_device, shift=shift), dk.summaries_of(b, min_qual), (on_device, shift, min_qual))


@pytest.mark.parametrize("on_device", [0, 1])
def test_summaries_of_long_reads_and_of_the_longest(bare, on_device):
    w = pw.workload()
    for packed in (False, True):
        _same_sums(_summary(bare, w.long, 15, on_device, packed=packed, shift=3), dw.single_sums("long"), ("long", on_device, packed))
    _same_sums(_summary(bare, w.main, 15, on_device, packed=True), dw.single_sums("main"), ("main packed", on_device))
    L = rlib.REAL_HIP_MAX_PATL_LONG
    one = types.SimpleNamespace(bases=np.zeros(L, dtype=np.uint8), qual=np.full(L, 63, dtype=np.uint8), offsets=np.array([0, L], dtype=np.uint64))
    got = _summary(bare, one, 63, on_device, shift=1)
    assert got["len"].tolist() == [L] and got["qsum"].tolist() == [L * 63] == [dw.MAX_QSUM]
    # a long read between short ones, in one wave
    rng = np.random.default_rng(4)
    lens = [40, 5000, 1, 321, 16384, 7]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    mix = types.SimpleNamespace(bases=np.zeros(int(off[-1]), dtype=np.uint8), qual=rng.integers(0, 64, size=int(off[-1])).astype(np.uint8), offsets=off)
    _same_sums(_summary(bare, mix, 20, on_device, shift=2), dk.summaries_of(mix, 20), ("mixed", on_device))


def test_summaries_without_qualities_uniform_length_and_empty(bare):
    import torch
    w = pw.workload()
    nq = types.SimpleNamespace(bases=w.main.bases, qual=None, offsets=w.main.offsets)
    for min_qual in (30, 31):
        for on_device in (0, 1):
            _same_sums(_summary(bare, nq, min_qual, on_device), dk.summaries(None, nq.offsets, min_qual), ("no qualities", min_qual, on_device))
    assert dk.summaries(None, nq.offsets, 31)["qsum"].max() == 0
    # uniform length: no offsets, with and without qualities, host and device
    patl, n = 37, 130
    rng = np.random.default_rng(6)
    bases, qual = rng.integers(0, 4, size=patl * n).astype(np.uint8), rng.integers(0, 64, size=patl * n).astype(np.uint8)
    off = (np.arange(n + 1) * patl).astype(np.uint64)
    for q in (qual, None):
        want = dk.summaries(q, off, 15)
        _same_sums(bare.read_summary(bases, q, patl=patl, min_qual=15), want, "uniform host")
        got = bare.read_summary(_dev(bases), None if q is None else _dev(q), patl=patl, min_qual=15)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32).reshape(-1, 2))
    # no reads at all
    empty = bare.read_summary(np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), offsets=np.zeros(1, dtype=np.uint64))
    assert empty.shape == (0,)
    bare.dup_stats(reset=True)
    with pytest.raises(rlib.RealHipError, match="min_qual") as e:
        bare.read_summary(bases, qual, patl=patl, min_qual=64)
    assert e.value.status == rlib.REAL_HIP_E_INVALID and bare.dup_stats()["launches"] == 0
    with pytest.raises(rlib.RealHipError, match="not monotone") as e:
        bare.read_summary(bases, qual, offsets=np.array([0, 10, 5], dtype=np.uint64))
    assert e.value.status == rlib.REAL_HIP_E_INVALID
    with pytest.raises(rlib.RealHipError, match="longer than") as e:
        bare.read_summary(bases, None, offsets=np.array([0, 16385], dtype=np.uint64))
    assert e.value.status == rlib.REAL_HIP_E_UNSUPPORTED and bare.dup_stats()["launches"] == 0


# ---- marking, single-end --------------------------------------------------------------------------------------------------
def _mark_single(m, info, sums, on_device, want=None):
    """one marking call and its statistics against the checker's"""
    if want is None:
        want = dk.mark_single(info, sums)
    m.dup_stats(reset=True)
    if on_device:
        dup = m.mark_duplicates(_dev(info), _dev_sums(sums)).cpu().numpy()
    else:
        dup = m.mark_duplicates(info, sums)
    st = m.dup_stats(reset=True)
    assert dup.dtype == np.uint8 and np.array_equal(dup, want[0]), np.nonzero(dup != want[0])[0][:10]
    assert {k: st[k] for k in dk.STATS} == want[1], (st, want[1])
    assert st["launches"] == (3 if info.shape[0] else 0) and (st["kernel_ms"] > 0 or not info.shape[0])
    assert m.dup_stats() == dict(st, reads=0, placed=0, groups=0, duplicates=0, launches=0, kernel_ms=0.0)       # reset
    return dup


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("which", ["main", "long"])
def test_marks_of_the_workload(ora, single, which, on_device):
    m, rec = single
    b = getattr(pw.workload(), which)
    sums = _summary(m, b, dw.MIN_QUAL, on_device)
    _same_sums(sums, dw.single_sums(which), which)
    info, _, wdup, wst, groups = dw.single_expected(ora, which)
    dup = _mark_single(m, rec[which], sums, on_device, (wdup, wst))
    assert int(dup.sum()) == (304 if which == "main" else 0)


@pytest.mark.parametrize("on_device", [0, 1])
def test_marks_of_hand_made_records(bare, on_device):
    info, sums, want = dw.hand_single()
    dup = _mark_single(bare, info, sums, on_device)
    assert dup.tolist() == want.tolist()
    # every record unplaced; one record; none
    none = np.array([dw._info(s, 1000) for s in (0, 3, 4, 0, 4)], dtype=np.uint64)
    assert _mark_single(bare, none, sums[:5], on_device).tolist() == [0] * 5
    assert _mark_single(bare, info[:1], sums[:1], on_device).tolist() == [0]
    assert _mark_single(bare, info[:0], sums[:0], on_device).shape == (0,)


def test_a_group_of_5000_copies_and_the_tie_rule(bare):
    """one site, both strands: more than a block and several tiles of the sort; many equal qsum"""
    rng = np.random.default_rng(8)
    n = 5000
    info = np.array([dw._info(1 + (i % 7 == 0), 777 if i % 7 else 777 - 49) for i in range(n)], dtype=np.uint64)
    sums = np.zeros(n, dtype=dk.SUM_DTYPE)
    sums["len"], sums["qsum"] = 50, rng.integers(1000, 1040, size=n)
    dup, st, groups = dk.mark_single(info, sums)
    assert st["groups"] == 2 and st["duplicates"] == n - 2 and (sums["qsum"] == sums["qsum"].max()).sum() > 50
    _mark_single(bare, info, sums, 0, (dup, st))
    _mark_single(bare, info, sums, 1, (dup, st))


def test_300000_records_and_their_shuffle(bare):
    """the sort's multi-block path; the marks of a shuffled order are the checker's for that order"""
    info, sums = dw.synthetic_records()
    first = _mark_single(bare, info, sums, 1)
    perm = np.random.default_rng(10).permutation(info.shape[0])
    second = _mark_single(bare, info[perm], sums[perm], 0)
    assert first.sum() == second.sum() and not np.array_equal(first[perm], second)      # (ties go to another copy in another order)


# ---- marking, paired-end --------------------------------------------------------------------------------------------------
def _lib_pairs(rec):
    pairs = np.zeros(rec.shape[0], dtype=rlib.PAIR_DTYPE)
    for k in rlib.PAIR_DTYPE.names:
        if k != "reserved":
            pairs[k] = rec[k]
    return pairs


def _mark_pairs(m, pairs, s1, s2, on_device, want=None):
    if want is None:
        want = dk.mark_pairs(pairs, s1, s2)
    m.dup_stats(reset=True)
    if on_device:
        dup = m.mark_duplicates_pairs(_dev(pairs.view(np.uint8).reshape(-1, 40)), _dev_sums(s1), _dev_sums(s2)).cpu().numpy()
    else:
        dup = m.mark_duplicates_pairs(pairs, s1, s2)
    st = m.dup_stats(reset=True)
    assert np.array_equal(dup, want[0]), np.nonzero(dup != want[0])[0][:10]
    assert {k: st[k] for k in dk.STATS} == want[1], (st, want[1])
    assert st["launches"] == (5 if pairs.shape[0] else 0)
    return dup


@pytest.mark.parametrize("on_device", [0, 1])
def test_marks_of_hand_made_pairs(bare, on_device):
    rec, s1, s2, want = dw.hand_pairs()
    pairs = _lib_pairs(rec)
    assert _mark_pairs(bare, pairs, s1, s2, on_device).tolist() == want.tolist()
    assert _mark_pairs(bare, pairs[8:10], s1[8:10], s2[8:10], on_device).tolist() == [0, 0]
    assert _mark_pairs(bare, pairs[:0], s1[:0], s2[:0], on_device).shape == (0,)


@pytest.mark.parametrize("on_device", [0, 1])
def test_marks_of_the_paired_workload(ora, on_device):
    """match_pairs on the derived workload, its records asserted to be the pair checker's; summaries of both mates; the marks"""
    dw.assert_pair_conditions(ora)
    g, b1, b2 = dw.pair_workload()
    rec, ws1, ws2, wdup, wst, groups = dw.pair_expected(ora)
    m = PairMatcher(RealOptions(seedl=iw.SEEDL, seedkmax=2, totalkmax=iw.TOTALK, scores=True, filter_level=iw.FILTER_LEVEL).normalise())
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    pairs = m.match_pairs(b1, b2, iw.WINDOW[0], iw.WINDOW[1])
    pc.assert_records_equal(pairs, rec, "match_pairs")
    s1, s2 = _summary(m, b1, dw.MIN_QUAL, on_device), _summary(m, b2, dw.MIN_QUAL, on_device)
    _same_sums(s1, ws1, "mate 1")
    _same_sums(s2, ws2, "mate 2")
    dup = _mark_pairs(m, pairs, s1, s2, on_device, (wdup, wst))
    assert int(dup.sum()) == 112
    m.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_marking_errors_are_loud_and_launch_nothing(bare):
    m = bare
    info, sums, _ = dw.hand_single()
    rec, s1, s2, _ = dw.hand_pairs()
    pairs = _lib_pairs(rec)
    dup = np.zeros(32, dtype=np.uint8)
    L, h = m._L, m._h
    m.dup_stats(reset=True)

    def refused(word, rc):
        with pytest.raises(rlib.RealHipError, match=word) as e:
            m._check(rc)
        assert e.value.status == rlib.REAL_HIP_E_INVALID
        st = m.dup_stats()
        assert st["launches"] == 0 and st["reads"] == 0, word

    n = info.shape[0]
    refused("null", L.real_hip_mark_duplicates(h, None, sums.ctypes.data, n, 0, dup.ctypes.data))
    refused("null", L.real_hip_mark_duplicates(h, info.ctypes.data, None, n, 0, dup.ctypes.data))
    refused("null", L.real_hip_mark_duplicates(h, info.ctypes.data, sums.ctypes.data, n, 0, None))
    refused("null", L.real_hip_mark_duplicates_pairs(h, None, s1.ctypes.data, s2.ctypes.data, 3, 0, dup.ctypes.data))
    refused("null", L.real_hip_mark_duplicates_pairs(h, pairs.ctypes.data, s1.ctypes.data, None, 3, 0, dup.ctypes.data))
    # more than 2^32 records: refused on the count alone (no array is looked at)
    refused("more than 2\\^32", L.real_hip_mark_duplicates(h, info.ctypes.data, sums.ctypes.data, (1 << 32) + 1, 0, dup.ctypes.data))
    refused("more than 2\\^32", L.real_hip_mark_duplicates_pairs(h, pairs.ctypes.data, s1.ctypes.data, s2.ctypes.data, (1 << 32) + 1, 0, dup.ctypes.data))
    st = rlib.RealHipDupStats()
    st.struct_size = C.sizeof(rlib.RealHipDupStats) - 8
    refused("struct_size", L.real_hip_dup_stats_get(h, C.byref(st), 0))
    big = rlib.RealHipBatch()
    big.struct_size = C.sizeof(rlib.RealHipBatch) - 4
    refused("struct_size", L.real_hip_read_summary(h, C.byref(big), 15, dup.ctypes.data))
    # n == 0 with null arrays is valid
    assert L.real_hip_mark_duplicates(h, None, None, 0, 0, None) == 0 and L.real_hip_mark_duplicates_pairs(h, None, None, None, 0, 1, None) == 0
    assert not dup.any()
