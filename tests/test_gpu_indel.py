"""Indel calls on the device (real_hip_indel_*) against the checker of indel_checker.py: the event list and the call list bit for
bit, and every counter -- on records written by hand (indel_workloads.hand_cases: the splits, gap lengths, read lengths, runs,
text edges, N bits, group sizes and refused records the kernels take another path at) and on records that are
real_hip_match_pairs_singles' and real_hip_gap_rescue's own (indel_workloads.planted)."""
import ctypes as C

import numpy as np
import pytest

import gap_checker as gc
import gap_workloads as gw
import indel_checker as ic
import indel_workloads as iw
import pileup_checker as pk
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions

pytestmark = pytest.mark.gpu

THRESHOLDS = (20, 2, 4)


def _matcher(sym, frag_start, fileid=0, index=False, seedkmax=2, totalkmax=gw.TOTALKMAX):
    m = PairMatcher(RealOptions(seedl=gw.SEEDL, seedkmax=seedkmax, totalkmax=totalkmax, scores=False, filter_level=0).normalise())
    m.set_text_symbols(fileid, sym, frag_start)
    if index:
        m.build_index_block()
    return m


_H, _WANT = {}, {}


def _hand():
    if not _H:
        _H.update(iw.hand_cases())
    return _H


def _want(min_qual=20, lo=0, hi=None, fileid=0, quals=True):
    """the checker's stage over the hand-made records [lo, hi): computed once per key, never changed"""
    h = _hand()
    hi = h["b1"].n_reads if hi is None else hi
    key = (min_qual, lo, hi, fileid, quals)
    if key not in _WANT:
        pu = pk.Pileup(h["sym"], fileid, min_qual)
        pu.add_pairs(h["pb1"], h["pb2"], h["pairs"])
        ind = ic.Indels(pu, h["frag_start"])
        b1, b2 = h["b1"].part(lo, hi), h["b2"].part(lo, hi)
        if not quals:
            b1, b2 = b1.without_qualities(), b2.without_qualities()
        ind.add(b1, b2, h["gaps"][lo:hi])
        _WANT[key] = ind
    return _WANT[key]


def _pileup(m, h, min_qual):
    m.pileup_begin(min_qual)
    m.pileup_add_pairs(h["pb1"], h["pb2"], h["pairs"])
    m.pileup_finish()


def _counters(st):
    return {k: st[k] for k in ic.COUNTERS + ("distinct", "calls", "het", "hom", "deletions", "insertions")}


def _check(m, want, thr=THRESHOLDS, what=""):
    """finish with thr, both lists and every counter against the checker"""
    n_ev, n_calls = m.indel_finish(*thr)
    ev, calls = m.indel_events(), m.indel_calls(cap=1)
    ic.assert_lists_equal(ev, want.events(*thr), what + " events")
    ic.assert_lists_equal(calls, want.calls(*thr), what + " calls")
    assert (n_ev, n_calls) == (ev.shape[0], calls.shape[0])
    st = m.indel_stats()
    assert _counters(st) == want.finish_stats(*thr), (what, st, want.finish_stats(*thr))
    return st


@pytest.mark.parametrize("min_qual", [0, 20])
def test_hand_made_records_against_the_checker(min_qual):
    h, want = _hand(), _want(min_qual)
    m = _matcher(h["sym"], h["frag_start"])
    _pileup(m, h, min_qual)
    m.indel_stats(reset=True)
    m.indel_begin()
    keep = h["gaps"].copy()
    m.indel_add(h["b1"], h["b2"], h["gaps"])
    st = _check(m, want, what="hand-made records, min_qual %d" % min_qual)
    print(st)
    assert keep.tobytes() == h["gaps"].tobytes(), "the records are inputs"
    assert st["launches"] == 1 + 8 + 3 and st["kernel_ms"] > 0
    f = want.finish_stats(*THRESHOLDS)
    assert f["invalid"] == 10 and f["other_file"] == 1 and f["ungapped"] == 1 and f["on_n"] == 3 and f["shift_capped"] >= 8 and f["shifted"] > 40
    assert (f["low_qual"] > 0) == (min_qual == 20) and f["deletions"] > 5 and f["insertions"] > 5 and f["het"] > 2 and f["hom"] > 2
    sizes = sorted(int(v) for v in m.indel_events()["alt_n"])
    assert sizes[-3:] == [64, 65, 300] and 1 in sizes and 2 in sizes
    m.indel_end()
    assert _counters(m.indel_stats(reset=True))["events"] == f["events"] and _counters(m.indel_stats())["events"] == 0
    m.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(n):
    h = _hand()
    lo = 330 - n // 2                                                  # (across the runs, the groups and the N bits)
    want = _want(20, lo, lo + n)
    m = _matcher(h["sym"], h["frag_start"])
    _pileup(m, h, 20)
    m.indel_begin()
    m.indel_add(h["b1"].part(lo, lo + n), h["b2"].part(lo, lo + n), h["gaps"][lo:lo + n])
    _check(m, want, what="n_reads %d" % n)
    m.close()


def test_adds_in_parts_finish_again_begin_again():
    h, want = _hand(), _want(20)
    b1, b2, gaps = h["b1"], h["b2"], h["gaps"]
    n = b1.n_reads
    m = _matcher(h["sym"], h["frag_start"])
    _pileup(m, h, 20)
    for cuts in ((0, n // 2 + 1, n), (0, 65, 400, n), (0, 0, n)):
        m.indel_stats(reset=True)
        m.indel_begin()                                                # (a second begin starts again)
        for a, b in zip(cuts[:-1], cuts[1:]):
            m.indel_add(b1.part(a, b), b2.part(a, b), gaps[a:b])
        _check(m, want, what="adds at %r" % (cuts,))
    # finish again with other thresholds: only the grouped events are read again
    launches = m.indel_stats()["launches"]
    for thr in ((0, 1, 0), (200, 2, 4), (20, 11, 4), (20, 2, 21), (1 << 31, 1, 0), THRESHOLDS):
        _check(m, want, thr, "thresholds %r" % (thr,))
    assert m.indel_stats()["launches"] <= launches + 6 * 3
    assert want.calls(0, 1, 0).shape[0] > want.calls(*THRESHOLDS).shape[0] > want.calls(200, 2, 4).shape[0] > 0 == want.calls(1 << 31, 1, 0).shape[0]
    # an add after a finish is out of turn; a new begin takes adds again
    with pytest.raises(rlib.RealHipError, match="add after finish"):
        m.indel_add(b1, b2, gaps)
    m.indel_begin()
    m.indel_stats(reset=True)
    m.indel_add(b1.part(0, 100), b2.part(0, 100), gaps[:100])
    _check(m, _want(20, 0, 100), what="begun again")
    m.close()


def test_device_arrays_packed_batches_and_no_qualities():
    import torch
    h, want = _hand(), _want(20)
    b1, b2, gaps = h["b1"], h["b2"], h["gaps"]
    m = _matcher(h["sym"], h["frag_start"])
    _pileup(m, h, 20)
    dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)]
    dgaps = torch.from_numpy(gaps.view(np.uint8).copy()).cuda()
    for what, g in (("device arrays", dgaps), ("device reads, host records", gaps)):
        m.indel_stats(reset=True)
        m.indel_begin()
        m.indel_add(dev[0], dev[1], g)
        _check(m, want, what=what)
    # the lists into device memory
    total = want.events(*THRESHOLDS).shape[0]
    out, n_out = torch.zeros(total * 8, dtype=torch.int32, device="cuda"), C.c_uint64(0)
    m._check(m._L.real_hip_indel_events(m._h, out.data_ptr(), total, C.byref(n_out), 1))
    ic.assert_lists_equal(out.cpu().numpy().view(rlib.INDEL_DTYPE), want.events(*THRESHOLDS), "events on the device")
    # packed batches whose reads start inside a byte
    keep, bb = [], []
    for b in (b1, b2):
        packed = synth.pack_bases(np.concatenate([np.zeros(1, np.uint8), b.bases]))
        qual, offs = np.concatenate([np.zeros(1, np.uint8), b.qual]), (b.offsets + np.uint64(1)).astype(np.uint64)
        bb.append(rlib.sized(rlib.RealHipBatch, on_device=0, n_reads=b.n_reads, bases=packed.ctypes.data, qual=qual.ctypes.data, offsets=offs.ctypes.data,
                             packed=1))
        keep += [packed, qual, offs]
    m.indel_stats(reset=True)
    m.indel_begin()
    m._check(m._L.real_hip_indel_add(m._h, C.byref(bb[0]), C.byref(bb[1]), gaps.ctypes.data))
    _check(m, want, what="packed, reads start inside a byte")
    # a batch without qualities counts as 30: nothing is of low quality, every q is 30
    wq = _want(20, quals=False)
    m.indel_stats(reset=True)
    m.indel_begin()
    m.indel_add(b1.without_qualities(), b2.without_qualities(), gaps)
    st = _check(m, wq, what="no qualities")
    ev = m.indel_events()
    assert st["low_qual"] == 0 and np.array_equal(ev["qsum"], 30 * ev["alt_n"])
    m.close()


def test_two_genome_files_and_zero_events():
    h = _hand()
    b1, b2 = h["b1"], h["b2"]
    m = _matcher(h["sym"], h["frag_start"], fileid=1)
    m.pileup_begin(20)
    m.pileup_add_pairs(h["pb1"], h["pb2"], h["pairs"])                # (the pair records are file 0's: nothing is piled up)
    m.pileup_finish()
    m.indel_begin()
    m.indel_add(b1, b2, h["gaps"])
    w1 = _want(20, fileid=1)
    st = _check(m, w1, what="file 1")
    assert st["placed"] == 1 and st["other_file"] == _want(20).stats["placed"] + _want(20).stats["invalid"] and st["distinct"] == 1
    # the records half and half; every list again
    gaps = h["gaps"].copy()
    gaps["fileid"][::2] = 1
    pu = pk.Pileup(h["sym"], 1, 20)
    ind = ic.Indels(pu, h["frag_start"])
    ind.add(b1, b2, gaps)
    m.indel_stats(reset=True)
    m.indel_begin()
    m.indel_add(b1, b2, gaps)
    st = _check(m, ind, what="mixed records, file 1")
    assert st["other_file"] > 200 and st["events"] > 200
    # zero events: no record is this file's; then no record at all, then no add
    gaps["fileid"][:] = 0
    for adds in ([(b1, b2, gaps)], [(b1.part(0, 0), b2.part(0, 0), gaps[:0])], []):
        m.indel_stats(reset=True)
        m.indel_begin()
        for a in adds:
            m.indel_add(*a)
        assert m.indel_finish(*THRESHOLDS) == (0, 0)
        assert m.indel_events().shape[0] == 0 and m.indel_calls().shape[0] == 0
        st = m.indel_stats()
        assert (st["events"], st["distinct"], st["calls"], st["placed"]) == (0, 0, 0, 0)
    m.close()


def test_capacity_protocol_and_loud_errors():
    import torch
    h, want = _hand(), _want(20)
    b1, b2, gaps = h["b1"], h["b2"], h["gaps"]
    m = _matcher(h["sym"], h["frag_start"])
    L, err = m._L, lambda: m._L.real_hip_last_error(m._h).decode()     # noqa: E731
    r1, r2 = m._mate_batch(b1), m._mate_batch(b2)
    n_out = C.c_uint64(0)
    prm = rlib.sized(rlib.RealHipIndelParams, min_call_qual=20, min_alt=2, min_depth=4)
    INV = rlib.REAL_HIP_E_INVALID
    # out of turn: no pileup, an unfinished pileup
    assert L.real_hip_indel_begin(m._h) == INV and "finished pileup" in err()
    m.pileup_begin(20)
    assert L.real_hip_indel_begin(m._h) == INV
    m.pileup_add_pairs(h["pb1"], h["pb2"], h["pairs"])
    m.pileup_finish()
    assert L.real_hip_indel_add(m._h, C.byref(r1), C.byref(r2), gaps.ctypes.data) == INV and "add without begin" in err()
    assert L.real_hip_indel_finish(m._h, C.byref(prm), None, None) == INV and "finish without begin" in err()
    assert L.real_hip_indel_events(m._h, None, 0, C.byref(n_out), 0) == INV and "before finish" in err()
    m.indel_begin()
    assert L.real_hip_indel_calls(m._h, None, 0, C.byref(n_out), 0) == INV and "before finish" in err()
    # bad arguments: nothing launched
    launches = m.indel_stats()["launches"]
    assert L.real_hip_indel_add(m._h, None, C.byref(r2), gaps.ctypes.data) == INV
    assert L.real_hip_indel_add(m._h, C.byref(r1), None, gaps.ctypes.data) == INV
    assert L.real_hip_indel_add(m._h, C.byref(r1), C.byref(r2), None) == INV and "null gaps" in err()
    short = m._mate_batch(b2.part(0, 5))
    assert L.real_hip_indel_add(m._h, C.byref(r1), C.byref(short), gaps.ctypes.data) == INV and "different numbers" in err()
    d2 = m._mate_batch(b2)
    d2.on_device = 2
    assert L.real_hip_indel_add(m._h, C.byref(r1), C.byref(d2), gaps.ctypes.data) == INV and "on_device" in err()
    big = m._mate_batch(b1)
    big.n_reads = d2.n_reads = (1 << 32) + 1
    d2.on_device = 0
    assert L.real_hip_indel_add(m._h, C.byref(big), C.byref(d2), gaps.ctypes.data) == INV and "2^32" in err()
    bad = rlib.sized(rlib.RealHipIndelParams, min_call_qual=20, min_alt=2, min_depth=4)
    bad.struct_size += 4
    assert L.real_hip_indel_finish(m._h, C.byref(bad), None, None) == INV and "struct_size" in err()
    assert L.real_hip_indel_finish(m._h, None, None, None) == INV
    st = rlib.sized(rlib.RealHipIndelStats)
    st.struct_size += 8
    assert L.real_hip_indel_stats_get(m._h, C.byref(st), 0) == INV
    assert m.indel_stats()["launches"] == launches, "nothing was launched"
    # the capacity protocol, on the host and on the device
    m.indel_add(b1, b2, gaps)
    m.indel_finish(*THRESHOLDS)
    for entry, recs in ((L.real_hip_indel_events, want.events(*THRESHOLDS)), (L.real_hip_indel_calls, want.calls(*THRESHOLDS))):
        total = recs.shape[0]
        out = np.full(total * 32, 0xAB, dtype=np.uint8)
        assert entry(m._h, out.ctypes.data, total - 1, C.byref(n_out), 0) == rlib.REAL_HIP_E_OVERFLOW
        assert n_out.value == total and (out == 0xAB).all()
        assert entry(m._h, None, 0, C.byref(n_out), 0) == rlib.REAL_HIP_E_OVERFLOW and n_out.value == total
        assert entry(m._h, out.ctypes.data, total, None, 0) == INV
        assert entry(m._h, out.ctypes.data, total, C.byref(n_out), 0) == rlib.REAL_HIP_OK
        ic.assert_lists_equal(out.view(rlib.INDEL_DTYPE), recs, "exact capacity")
        dout = torch.full((total * 32,), 0xAB, dtype=torch.uint8, device="cuda")
        assert entry(m._h, dout.data_ptr(), total - 1, C.byref(n_out), 1) == rlib.REAL_HIP_E_OVERFLOW
        assert n_out.value == total and bool((dout == 0xAB).all())
        assert entry(m._h, dout.data_ptr(), total + 3, C.byref(n_out), 1) == rlib.REAL_HIP_OK and n_out.value == total
        ic.assert_lists_equal(dout.cpu().numpy().view(rlib.INDEL_DTYPE), recs, "device list")
    # a text of another size or file id under the stage
    m.set_text_symbols(1, h["sym"], h["frag_start"])
    assert L.real_hip_indel_finish(m._h, C.byref(prm), None, None) == INV and "text was replaced" in err()
    assert L.real_hip_indel_begin(m._h) == INV
    m.set_text_symbols(0, h["sym"][:-7], [0, iw.HAND_CUT, h["sym"].shape[0] - 7])
    assert L.real_hip_indel_begin(m._h) == INV and "text was replaced" in err()
    m.set_text_symbols(0, h["sym"], h["frag_start"])
    _check(m, want, what="the text back")
    m.close()


def test_the_pileups_end_and_a_new_pileup_end_the_stage():
    h, want = _hand(), _want(20)
    m = _matcher(h["sym"], h["frag_start"])
    n_out = C.c_uint64(0)
    for ender in (m.pileup_end, lambda: m.pileup_begin(20), m.indel_end):
        _pileup(m, h, 20)
        m.indel_begin()
        m.indel_add(h["b1"], h["b2"], h["gaps"])
        m.indel_finish(*THRESHOLDS)
        ender()
        assert m._L.real_hip_indel_events(m._h, None, 0, C.byref(n_out), 0) == rlib.REAL_HIP_E_INVALID
        with pytest.raises(rlib.RealHipError):
            m.indel_add(h["b1"], h["b2"], h["gaps"])
    _pileup(m, h, 20)
    m.indel_stats(reset=True)
    m.indel_begin()
    m.indel_add(h["b1"], h["b2"], h["gaps"])
    _check(m, want, what="after the ends")
    m.close()


def test_planted_workload_on_the_matchers_and_the_rescues_own_records():
    w = iw.planted()
    g = w.g
    m = _matcher(g.sym, g.frag_start, index=True, seedkmax=iw.SEEDKMAX, totalkmax=iw.TOTALKMAX)
    pairs, s1, s2 = m.match_pairs_singles(w.b1, w.b2, w.min_ins, w.max_ins)
    gaps = m.gap_rescue(w.b1, w.b2, pairs, s1, s2, w.min_ins, w.max_ins, **w.prm._asdict())
    rec = np.zeros(gaps.shape[0], dtype=gc.REC_DTYPE)
    for k in gc.REC_DTYPE.names:
        rec[k] = gaps[k]
    m.pileup_begin(20)
    m.pileup_add_pairs(w.b1, w.b2, pairs)
    m.pileup_finish()
    pu = pk.Pileup(g.sym, 0, 20)
    pu.add_pairs(w.b1, w.b2, pairs)
    assert np.array_equal(m.pileup_depth(0, g.n), pu.depth)
    want = ic.Indels(pu, g.frag_start)
    want.add(w.b1, w.b2, rec)
    m.indel_begin()
    half = w.b1.n_reads // 2
    m.indel_add(w.b1.part(0, half), w.b2.part(0, half), gaps[:half])
    m.indel_add(w.b1.part(half, w.b1.n_reads), w.b2.part(half, w.b1.n_reads), gaps[half:])
    st = _check(m, want, what="planted")
    print(st)
    assert st["invalid"] == 0 and st["other_file"] == 0 and st["on_n"] == 0 and st["placed"] == m.gap_stats()["unique"]
    assert st["events"] > 200 and st["calls"] >= 12 and st["het"] >= 4 and st["hom"] >= 4 and st["deletions"] >= 4 and st["insertions"] >= 4
    # the planted indels the device calls, under their left-normalised names
    calls = {(int(c["pos"]), int(c["gap"]), int(c["seq"])): int(c["gt"]) for c in m.indel_calls()}
    right = sum(calls.get(iw.planted_key(w, p)) == (2 if p["hom"] else 1) for p in w.plants)
    print("planted genotypes called right: %d of %d" % (right, len(w.plants)))
    assert right >= 0.8 * len(w.plants)
    m.close()
