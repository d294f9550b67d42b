"""Gapped placements in the pileup and the calls on the device (real_hip_pileup_add_gapped, real_hip_call_add_gapped,
real_hip_pileup_depth_gapped) against the checker of pileup_gapped_checker.py: depth, gdepth, sites, evidence, calls and every
counter bit for bit -- on records written by hand (pileup_gapped_workloads.hand_cases: the lengths, splits, gap lengths, text
word offsets, text edges, N bits, strands, targets and refused records the kernels take another path at) and on records that are
real_hip_gap_rescue's and real_hip_match_gapped's own."""
import ctypes as C

import numpy as np
import pytest

import gap_checker as gc
import gap_workloads as gw
import indel_checker as ic
import indel_workloads as iw
import pileup_gapped_checker as pgc
import pileup_gapped_workloads as pgw
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions

pytestmark = pytest.mark.gpu

_H, _WANT = {}, {}


def _matcher(sym, frag_start, fileid=0, index=False, seedkmax=2, totalkmax=gw.TOTALKMAX):
    m = PairMatcher(RealOptions(seedl=gw.SEEDL, seedkmax=seedkmax, totalkmax=totalkmax, scores=False, filter_level=0).normalise())
    m.set_text_symbols(fileid, sym, frag_start)
    if index:
        m.build_index_block()
    return m


def _hand():
    if not _H:
        _H.update(pgw.hand_cases())
    return _H


def _want(min_qual=20, lo=0, hi=None, fileid=0, quals=True, pairs=True, gapped=True):
    """the checker's pileup and calls over the hand-made pair records and gap records [lo, hi): computed once per key, never changed"""
    h = _hand()
    hi = h["b1"].n_reads if hi is None else hi
    key = (min_qual, lo, hi, fileid, quals, pairs, gapped)
    if key not in _WANT:
        b1, b2 = h["b1"].part(lo, hi), h["b2"].part(lo, hi)
        if not quals:
            b1, b2 = b1.without_qualities(), b2.without_qualities()
        pu = pgc.GappedPileup(h["sym"], fileid, min_qual)
        if pairs:
            pu.add_pairs(h["pb1"], h["pb2"], h["pairs"])
        if gapped:
            pu.add_gapped(b1, b2, h["gaps"][lo:hi])
        cl = pgc.GappedCalls(pu)
        if pairs:
            cl.add_pairs(h["pb1"], h["pb2"], h["pairs"])
        if gapped:
            cl.add_gapped(b1, b2, h["gaps"][lo:hi])
        _WANT[key] = (pu, cl)
    return _WANT[key]


def _counters(st, names):
    return {k: int(st[k]) for k in names}


def _check_pileup(m, pu, what=""):
    """the finished pileup against the checker: depth, gdepth, sites, every counter"""
    n = pu.n
    assert np.array_equal(m.pileup_depth(0, n), pu.depth), what + " depth"
    assert np.array_equal(m.pileup_depth_gapped(0, n), pu.gdepth), what + " gdepth"
    sites, want = m.pileup_sites(), pu.sites()
    assert sites.shape == want.shape and sites.tobytes() == want.tobytes(), what + " sites"
    st, gst = m.pileup_stats(), m.pileup_gapped_stats()
    assert _counters(st, pu.finish_stats()) == pu.finish_stats(), (what, st, pu.finish_stats())
    assert _counters(gst, pgc.COUNTERS) == pu.gapped_stats(), (what, gst, pu.gapped_stats())
    assert int(pu.depth.sum()) == st["bases"] + gst["aligned_bases"], "the sum of depth[] equals bases + aligned_bases"
    return gst


def _check_calls(m, cl, what="", thr=(20, 4)):
    m.call_finish(*thr)
    ev, want = m.call_evidence(), cl.evidence()
    assert ev.shape == want.shape and ev.tobytes() == want.tobytes(), what + " evidence"
    calls, wc = m.call_variants(), cl.calls(*thr)
    assert calls.shape == wc.shape and calls.tobytes() == wc.tobytes(), what + " calls"
    st, gst = m.call_stats(), m.pileup_gapped_stats()
    assert _counters(st, cl.finish_stats(*thr)) == cl.finish_stats(*thr), (what, st, cl.finish_stats(*thr))
    assert _counters(gst, pgc.CALL_COUNTERS) == cl.gstats, (what, gst, cl.gstats)
    sites = m.pileup_sites()
    for b in range(4):
        sel = sites["ref"] != b
        assert np.array_equal(ev["cnt"][sel, b], sites["alt"][sel, b]), "cnt[s][b] == site.alt[b] for b != ref"


def _reset(m):
    m.pileup_stats(reset=True), m.call_stats(reset=True), m.pileup_gapped_stats(reset=True)


def _run(m, h, min_qual, adds, call_adds=None):
    """begin, the adds in their order, finish; call_begin, the call adds (default: the same), left unfinished"""
    _reset(m)
    m.pileup_begin(min_qual)
    for kind, *a in adds:
        (m.pileup_add_pairs if kind == "pairs" else m.pileup_add_gapped)(*a)
    m.pileup_finish()
    m.call_begin()
    for kind, *a in (adds if call_adds is None else call_adds):
        (m.call_add_pairs if kind == "pairs" else m.call_add_gapped)(*a)


@pytest.mark.parametrize("min_qual", [0, 20])
def test_hand_made_records_against_the_checker(min_qual):
    h = _hand()
    pu, cl = _want(min_qual)
    m = _matcher(h["sym"], h["frag_start"])
    keep = h["gaps"].copy()
    _run(m, h, min_qual, [("pairs", h["pb1"], h["pb2"], h["pairs"]), ("gapped", h["b1"], h["b2"], h["gaps"])])
    gst = _check_pileup(m, pu, "hand-made records, min_qual %d" % min_qual)
    _check_calls(m, cl, "hand-made records, min_qual %d" % min_qual)
    gst = m.pileup_gapped_stats()
    print(gst)
    assert keep.tobytes() == h["gaps"].tobytes(), "the records are inputs"
    assert gst["launches"] == 2 and gst["kernel_ms"] > 0 and gst["records"] == h["gaps"].shape[0]
    assert gst["invalid"] == 11 and gst["other_file"] == 1 and gst["ungapped"] >= 20 and gst["deleted"] > 0 and gst["inserted"] > 0
    assert gst["n_dropped"] > 0 and (gst["low_qual"] > 0) == (min_qual == 20) and (gst["site_low_qual"] > 0) == (min_qual == 20)
    assert gst["site_bases"] > gst["mismatches"] > 500, "reads that show the text's base on a site count as evidence"
    m.pileup_end()
    assert m.pileup_gapped_stats(reset=True)["placed"] == pu.gstats["placed"] and m.pileup_gapped_stats()["placed"] == 0
    m.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_batch_sizes(n):
    h = _hand()
    lo = 200 - n // 2
    pu, cl = _want(20, lo, lo + n)
    m = _matcher(h["sym"], h["frag_start"])
    part = ("gapped", h["b1"].part(lo, lo + n), h["b2"].part(lo, lo + n), h["gaps"][lo:lo + n])
    _run(m, h, 20, [("pairs", h["pb1"], h["pb2"], h["pairs"]), part])
    _check_pileup(m, pu, "n_reads %d" % n)
    _check_calls(m, cl, "n_reads %d" % n)
    m.close()


def test_adds_in_parts_interleaved_in_any_order_give_one_result():
    h = _hand()
    pu, cl = _want(20)
    b1, b2, gaps, n = h["b1"], h["b2"], h["gaps"], h["b1"].n_reads
    pb1, pb2, pairs, np_ = h["pb1"], h["pb2"], h["pairs"], h["pb1"].n_reads
    m = _matcher(h["sym"], h["frag_start"])

    def g(a, b):
        return ("gapped", b1.part(a, b), b2.part(a, b), gaps[a:b])

    def p(a, b):
        return ("pairs", pb1.part(a, b), pb2.part(a, b), pairs[a:b])
    orders = ([g(0, n // 2 + 1), p(0, np_), g(n // 2 + 1, n)],
              [g(0, 65), p(0, 64), g(65, 400), p(64, np_), g(400, n)],
              [g(0, 0), g(0, n), p(0, np_), g(n, n)])
    for k, adds in enumerate(orders):
        _run(m, h, 20, adds, call_adds=adds[::-1])
        _check_pileup(m, pu, "order %d" % k)
        _check_calls(m, cl, "order %d" % k)
    m.close()


def test_device_arrays_mixed_arrays_packed_batches_and_no_qualities():
    import torch
    h = _hand()
    pu, cl = _want(20)
    b1, b2, gaps = h["b1"], h["b2"], h["gaps"]
    pairs_add = ("pairs", h["pb1"], h["pb2"], h["pairs"])
    m = _matcher(h["sym"], h["frag_start"])
    dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)]
    dgaps = torch.from_numpy(gaps.view(np.uint8).copy()).cuda()
    for what, g in (("device arrays", dgaps), ("device reads, host records", gaps)):
        _run(m, h, 20, [pairs_add, ("gapped", dev[0], dev[1], g)])
        _check_pileup(m, pu, what)
        _check_calls(m, cl, what)
    # gdepth into device memory
    out = torch.full((pu.n,), 7, dtype=torch.int32, device="cuda")
    m.pileup_depth_gapped(0, pu.n, out=out)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), pu.gdepth)
    assert np.array_equal(m.pileup_depth_gapped(31, 1000), pu.gdepth[31:1031])
    # packed batches whose reads start inside a byte
    keep, bb = [], []
    for b in (b1, b2):
        packed = synth.pack_bases(np.concatenate([np.zeros(1, np.uint8), b.bases]))
        qual, offs = np.concatenate([np.zeros(1, np.uint8), b.qual]), (b.offsets + np.uint64(1)).astype(np.uint64)
        bb.append(rlib.sized(rlib.RealHipBatch, on_device=0, n_reads=b.n_reads, bases=packed.ctypes.data, qual=qual.ctypes.data, offsets=offs.ctypes.data,
                             packed=1))
        keep += [packed, qual, offs]
    _reset(m)
    m.pileup_begin(20)
    m.pileup_add_pairs(*pairs_add[1:])
    m._check(m._L.real_hip_pileup_add_gapped(m._h, C.byref(bb[0]), C.byref(bb[1]), gaps.ctypes.data))
    m.pileup_finish()
    m.call_begin()
    m.call_add_pairs(*pairs_add[1:])
    m._check(m._L.real_hip_call_add_gapped(m._h, C.byref(bb[0]), C.byref(bb[1]), gaps.ctypes.data))
    _check_pileup(m, pu, "packed, reads start inside a byte")
    _check_calls(m, cl, "packed, reads start inside a byte")
    # a batch without qualities counts as 30: nothing is of low quality
    pq, cq = _want(20, quals=False)
    _run(m, h, 20, [pairs_add, ("gapped", b1.without_qualities(), b2.without_qualities(), gaps)])
    gst = _check_pileup(m, pq, "no qualities")
    _check_calls(m, cq, "no qualities")
    assert gst["low_qual"] == 0 and m.pileup_gapped_stats()["site_low_qual"] == 0
    m.close()


def test_the_indel_calls_do_not_move_and_no_gapped_add_reads_zeros():
    h = iw.hand_cases()
    thr = (20, 2, 4)
    m = _matcher(h["sym"], h["frag_start"])
    got = []
    for with_gapped in (False, True):
        m.pileup_begin(20)
        m.pileup_add_pairs(h["pb1"], h["pb2"], h["pairs"])
        if with_gapped:
            m.pileup_add_gapped(h["b1"], h["b2"], h["gaps"])
        m.pileup_finish()
        gd = m.pileup_depth_gapped(0, h["sym"].shape[0])
        assert bool(gd.any()) == with_gapped, "zeros when no gapped add was made"
        m.indel_begin()
        m.indel_add(h["b1"], h["b2"], h["gaps"])
        m.indel_finish(*thr)
        got.append((m.indel_events(), m.indel_calls(), m.pileup_depth(0, h["sym"].shape[0]), gd))
    (e0, c0, d0, g0), (e1, c1, d1, g1) = got
    ic.assert_lists_equal(e1, e0, "events with and without the gapped adds")
    ic.assert_lists_equal(c1, c0, "calls with and without the gapped adds")
    assert e0.shape[0] > 50 and c0.shape[0] > 5 and np.array_equal(d1 - g1, d0) and not np.array_equal(d1, d0)
    # and they are the checker's
    pu = pgc.GappedPileup(h["sym"], 0, 20)
    pu.add_pairs(h["pb1"], h["pb2"], h["pairs"])
    pu.add_gapped(h["b1"], h["b2"], h["gaps"])
    assert np.array_equal(d1, pu.depth) and np.array_equal(g1, pu.gdepth)
    want = ic.Indels(pu.ungapped_view(), h["frag_start"])
    want.add(h["b1"], h["b2"], h["gaps"])
    ic.assert_lists_equal(e1, want.events(*thr), "events against the checker on depth - gdepth")
    m.close()


def test_two_genome_files():
    h = _hand()
    b1, b2 = h["b1"], h["b2"]
    gaps = h["gaps"].copy()
    gaps["fileid"][::2] = 1
    pairs = h["pairs"].copy()
    pairs["fileid"][::3] = 1
    m = _matcher(h["sym"], h["frag_start"], fileid=1)
    for fileid in (1, 0):
        m.set_text_symbols(fileid, h["sym"], h["frag_start"])
        pu = pgc.GappedPileup(h["sym"], fileid, 20)
        pu.add_pairs(h["pb1"], h["pb2"], pairs)
        pu.add_gapped(b1, b2, gaps)
        cl = pgc.GappedCalls(pu)
        cl.add_pairs(h["pb1"], h["pb2"], pairs)
        cl.add_gapped(b1, b2, gaps)
        _run(m, h, 20, [("pairs", h["pb1"], h["pb2"], pairs), ("gapped", b1, b2, gaps)])
        gst = _check_pileup(m, pu, "file %d" % fileid)
        _check_calls(m, cl, "file %d" % fileid)
        assert gst["other_file"] > 150 and gst["placed"] > 150                 # (about half of the 400 fitting records each)
    m.close()


def test_the_rescues_own_records_on_the_planted_workload():
    w = iw.planted()
    g = w.g
    m = _matcher(g.sym, g.frag_start, index=True, seedkmax=iw.SEEDKMAX, totalkmax=iw.TOTALKMAX)
    pairs, s1, s2 = m.match_pairs_singles(w.b1, w.b2, w.min_ins, w.max_ins)
    gaps = m.gap_rescue(w.b1, w.b2, pairs, s1, s2, w.min_ins, w.max_ins, **w.prm._asdict())
    rec = np.zeros(gaps.shape[0], dtype=gc.REC_DTYPE)
    for k in gc.REC_DTYPE.names:
        rec[k] = gaps[k]
    pu = pgc.GappedPileup(g.sym, 0, 20)
    pu.add_pairs(w.b1, w.b2, pairs)
    pu.add_gapped(w.b1, w.b2, rec)
    cl = pgc.GappedCalls(pu)
    cl.add_pairs(w.b1, w.b2, pairs)
    cl.add_gapped(w.b1, w.b2, rec)
    half = w.b1.n_reads // 2
    parts = [("gapped", w.b1.part(0, half), w.b2.part(0, half), gaps[:half]), ("pairs", w.b1, w.b2, pairs),
             ("gapped", w.b1.part(half, w.b1.n_reads), w.b2.part(half, w.b1.n_reads), gaps[half:])]
    _run(m, None, 20, parts)
    gst = _check_pileup(m, pu, "planted")
    _check_calls(m, cl, "planted")
    print(gst)
    assert gst["invalid"] == 0 and gst["other_file"] == 0 and gst["placed"] == m.gap_stats()["unique"] > 200
    assert gst["deleted"] > 100 and gst["inserted"] > 100
    # what the stage is for: beside a planted homozygous deletion the depth comes back
    depth, gdepth = m.pileup_depth(0, g.n).astype(np.int64), m.pileup_depth_gapped(0, g.n).astype(np.int64)
    seen = 0
    for p in w.plants:
        if p["cls"] == "hom_del" and p["g"] >= 2:
            flank = np.r_[p["x"] - 30:p["x"] - 5]
            assert depth[flank].mean() > (depth - gdepth)[flank].mean() + 3
            seen += 1
    assert seen >= 3
    m.close()


def test_match_gappeds_own_records_the_single_end_batch_given_twice():
    import gap_anchor_workloads as aw
    w = aw.workload()
    g, b = w["g"], w["b"]
    m = PairMatcher(RealOptions(seedl=w["seedl"], seedkmax=2, totalkmax=aw.TOTALKMAX, scores=False, filter_level=0).normalise())
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    info, _ = m.match_unique(b.bases, b.qual, b.offsets)
    gaps = m.match_gapped(b, max(w["seedl"], aw.default_anchor(w["patl"], w["prm"])), info=info, **w["prm"]._asdict())
    rec = np.zeros(gaps.shape[0], dtype=gc.REC_DTYPE)
    for k in gc.REC_DTYPE.names:
        rec[k] = gaps[k]
    pu = pgc.GappedPileup(g.sym, 0, 20)
    pu.add(b, info)
    pu.add_gapped(b, b, rec)
    cl = pgc.GappedCalls(pu)
    cl.add(b, info)
    cl.add_gapped(b, b, rec)
    _reset(m)
    m.pileup_begin(20)
    m.pileup_add(b.bases, b.qual, info, offsets=b.offsets)
    m.pileup_add_gapped(b, b, gaps)
    m.pileup_finish()
    m.call_begin()
    m.call_add_gapped(b, b, gaps)
    m.call_add(b.bases, b.qual, info, offsets=b.offsets)
    gst = _check_pileup(m, pu, "single-end")
    _check_calls(m, cl, "single-end")
    print(gst)
    assert gst["placed"] > 20 and gst["deleted"] > 0 and gst["inserted"] > 0 and gst["invalid"] == 0
    m.close()


def test_every_listed_error_is_raised_and_nothing_is_launched():
    h = _hand()
    pu, cl = _want(20)
    b1, b2, gaps = h["b1"], h["b2"], h["gaps"]
    m = _matcher(h["sym"], h["frag_start"])
    L, err = m._L, lambda: m._L.real_hip_last_error(m._h).decode()      # noqa: E731
    r1, r2 = m._mate_batch(b1), m._mate_batch(b2)
    INV = rlib.REAL_HIP_E_INVALID
    add, cadd = L.real_hip_pileup_add_gapped, L.real_hip_call_add_gapped
    _reset(m)
    # out of turn
    assert add(m._h, C.byref(r1), C.byref(r2), gaps.ctypes.data) == INV and "add without begin" in err()
    assert cadd(m._h, C.byref(r1), C.byref(r2), gaps.ctypes.data) == INV and "add without begin" in err()
    assert L.real_hip_pileup_depth_gapped(m._h, 0, 1, None, 0) == INV and "before finish" in err()
    m.pileup_begin(20)
    assert L.real_hip_pileup_depth_gapped(m._h, 0, 1, None, 0) == INV and "before finish" in err()
    # bad arguments
    for entry in (add,):
        assert entry(m._h, None, C.byref(r2), gaps.ctypes.data) == INV
        assert entry(m._h, C.byref(r1), None, gaps.ctypes.data) == INV
        assert entry(m._h, C.byref(r1), C.byref(r2), None) == INV and "null gaps" in err()
        short = m._mate_batch(b2.part(0, 5))
        assert entry(m._h, C.byref(r1), C.byref(short), gaps.ctypes.data) == INV and "different numbers" in err()
        d2 = m._mate_batch(b2)
        d2.on_device = 2
        assert entry(m._h, C.byref(r1), C.byref(d2), gaps.ctypes.data) == INV and "on_device" in err()
        big = m._mate_batch(b1)
        big.n_reads = d2.n_reads = (1 << 32) + 1
        d2.on_device = 0
        assert entry(m._h, C.byref(big), C.byref(d2), gaps.ctypes.data) == INV and "2^32" in err()
    # a text of another file id or size under the pileup
    m.set_text_symbols(1, h["sym"], h["frag_start"])
    assert add(m._h, C.byref(r1), C.byref(r2), gaps.ctypes.data) == INV and "text was replaced" in err()
    m.set_text_symbols(0, h["sym"][:-7], [0, h["sym"].shape[0] - 7])
    assert add(m._h, C.byref(r1), C.byref(r2), gaps.ctypes.data) == INV and "text was replaced" in err()
    m.set_text_symbols(0, h["sym"], h["frag_start"])
    st = rlib.sized(rlib.RealHipPileupGappedStats)
    st.struct_size += 8
    assert L.real_hip_pileup_gapped_stats_get(m._h, C.byref(st), 0) == INV and "struct_size" in err()
    assert m.pileup_gapped_stats()["launches"] == 0 and m.pileup_gapped_stats()["records"] == 0, "nothing was launched"
    # n_reads == 0 is valid, with null gaps too
    e1, e2 = m._mate_batch(b1.part(0, 0)), m._mate_batch(b2.part(0, 0))
    assert add(m._h, C.byref(e1), C.byref(e2), None) == rlib.REAL_HIP_OK
    # the call leg: before the pileup's finish, then the same bad arguments, then after the calls' finish
    m.pileup_add_pairs(h["pb1"], h["pb2"], h["pairs"])
    m.pileup_add_gapped(b1, b2, gaps)
    assert cadd(m._h, C.byref(r1), C.byref(r2), gaps.ctypes.data) == INV and "add without begin" in err()
    m.pileup_finish()
    assert add(m._h, C.byref(r1), C.byref(r2), gaps.ctypes.data) == INV and "add after finish" in err()
    assert cadd(m._h, C.byref(r1), C.byref(r2), gaps.ctypes.data) == INV and "add without begin" in err()
    m.call_begin()
    launches = m.pileup_gapped_stats()["launches"]
    assert cadd(m._h, None, C.byref(r2), gaps.ctypes.data) == INV
    assert cadd(m._h, C.byref(r1), C.byref(r2), None) == INV and "null gaps" in err()
    assert cadd(m._h, C.byref(r1), C.byref(short), gaps.ctypes.data) == INV and "different numbers" in err()
    assert cadd(m._h, C.byref(big), C.byref(d2), gaps.ctypes.data) == INV and "2^32" in err()
    d2.n_reads, d2.on_device = r1.n_reads, 2
    assert cadd(m._h, C.byref(r1), C.byref(d2), gaps.ctypes.data) == INV and "on_device" in err()
    m.set_text_symbols(1, h["sym"], h["frag_start"])
    assert cadd(m._h, C.byref(r1), C.byref(r2), gaps.ctypes.data) == INV and "text was replaced" in err()
    m.set_text_symbols(0, h["sym"], h["frag_start"])
    assert cadd(m._h, C.byref(e1), C.byref(e2), None) == rlib.REAL_HIP_OK
    assert m.pileup_gapped_stats()["launches"] == launches, "nothing was launched"
    # the window checks of the depth
    n = pu.n
    out = np.zeros(4, np.uint32)
    assert L.real_hip_pileup_depth_gapped(m._h, n - 3, 4, out.ctypes.data, 0) == INV and "beyond the text" in err()
    assert L.real_hip_pileup_depth_gapped(m._h, n + 1, 0, out.ctypes.data, 0) == INV
    assert L.real_hip_pileup_depth_gapped(m._h, 0, 4, None, 0) == INV and "null depth" in err()
    assert L.real_hip_pileup_depth_gapped(m._h, n, 0, None, 0) == rlib.REAL_HIP_OK
    assert np.array_equal(m.pileup_depth_gapped(n - 4, 4), pu.gdepth[n - 4:])
    # the stage still works: the whole result
    m.call_add_pairs(h["pb1"], h["pb2"], h["pairs"])
    m.call_add_gapped(b1, b2, gaps)
    _check_pileup(m, pu, "behind the errors")
    _check_calls(m, cl, "behind the errors")
    assert cadd(m._h, C.byref(r1), C.byref(r2), gaps.ctypes.data) == INV and "add after finish" in err()
    # the pileup's end and a new begin release the second array: zeros again
    m.pileup_begin(20)
    m.pileup_add_pairs(h["pb1"], h["pb2"], h["pairs"])
    m.pileup_finish()
    assert not m.pileup_depth_gapped(0, n).any()
    m.pileup_end()
    assert L.real_hip_pileup_depth_gapped(m._h, 0, 1, out.ctypes.data, 0) == INV
    m.close()
