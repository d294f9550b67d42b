"""The four stages that consume gap records -- the gapped mismatch lists, the pileup's and the calls' gapped adds and the indel
calls -- agree on WHICH records they place: all four take a record to a placement with the one step of
real_amd/csrc/read_walk.h (placed_gap, on the decoder and the geometry rule of final_record.h), stage reads and records with one
function of real_hip_api.hip and keep their state in records of their own inside the ctx (real_hip_ctx.h).

(a) the hand-written records of pileup_gapped_workloads.hand_cases -- every refused record among them -- through all four, from
    host arrays and from device arrays: `placed`, `other_file` and `invalid` equal among the stages and equal to the three
    checkers'.  The text is one fragment, so the indel stage's fragment rule adds nothing.
(b) two contexts that have each run a mapping quality fold, a gap rescue, an indel add and a gapped pileup add: destroying one
    leaves the other's four statistics as they were and the other at work; a context made afterwards reads zeros.
(c) the three entry points refuse null gaps, misaligned device gaps and disagreeing mates with the code and the message they
    had before they shared their staging.
No oracle: the records of (a) are written by hand, (b) compares a context with itself."""
import ctypes as C

import numpy as np
import pytest

import gap_workloads as gw
import gapped_list_checker as glc
import indel_checker as ic
import pileup_gapped_checker as pgc
import pileup_gapped_workloads as pgw
from real_amd import lib as rlib
from real_amd.matcher import PairMatcher, RealOptions

pytestmark = pytest.mark.gpu

SHARED = ("placed", "other_file", "invalid")
MIN_QUAL = 20


def _matcher(sym, frag_start, index=False):
    m = PairMatcher(RealOptions(seedl=gw.SEEDL, seedkmax=2, totalkmax=gw.TOTALKMAX, scores=False, filter_level=0).normalise())
    m.set_text_symbols(0, sym, frag_start)
    if index:
        m.build_index_block()
    return m


@pytest.fixture(scope="module")
def hand():
    """the hand cases and what the three checkers count on them, computed once and left unchanged"""
    h = pgw.hand_cases()
    pu = pgc.GappedPileup(h["sym"], 0, MIN_QUAL)
    pu.add_pairs(h["pb1"], h["pb2"], h["pairs"])
    pu.add_gapped(h["b1"], h["b2"], h["gaps"])
    ind = ic.Indels(pu.ungapped_view(), h["frag_start"])
    ind.add(h["b1"], h["b2"], h["gaps"])
    lists = glc.gapped_lists(h["sym"], 0, h["b1"], h["b2"], h["gaps"])
    want = {k: int(pu.gapped_stats()[k]) for k in SHARED}
    assert want == {k: int(ind.stats[k]) for k in SHARED} == {k: int(lists[2][k]) for k in SHARED}, "the three checkers agree"
    refused = [v for v in pgw.EMPTY_NOTES.values()]
    assert want["invalid"] == refused.count("invalid") == 11 and want["other_file"] == refused.count("other_file") == 1 and want["placed"] > 400
    return dict(h, want=want, lists=lists)


def _four_stages(m, h, mates, gaps):
    """the lists, the pileup's add, the calls' add on the finished pileup, the indel add on it -> the four statistics"""
    for reset in (m.gapped_list_stats, m.pileup_gapped_stats, m.indel_stats):
        reset(reset=True)
    got = m.mismatches_gapped(*mates, gaps, cap=1 << 16)
    gl = m.gapped_list_stats()
    m.pileup_begin(MIN_QUAL)
    m.pileup_add_pairs(h["pb1"], h["pb2"], h["pairs"])
    m.pileup_add_gapped(*mates, gaps)
    m.pileup_finish()
    pg = m.pileup_gapped_stats(reset=True)
    m.call_begin()
    m.call_add_gapped(*mates, gaps)
    cg = m.pileup_gapped_stats()         # (the call leg counts site_bases alone: it places what the pileup leg placed, or the evidence differs)
    m.indel_begin()
    m.indel_add(*mates, gaps)
    idl = m.indel_stats()
    m.indel_end()
    m.call_end()
    m.pileup_end()
    return got, gl, pg, cg, idl


@pytest.mark.parametrize("where", ["host", "device"])
def test_the_four_stages_place_the_same_records(hand, where):
    h, want = hand, hand["want"]
    n = int(h["gaps"].shape[0])
    m = _matcher(h["sym"], h["frag_start"])
    mates, gaps = (h["b1"], h["b2"]), h["gaps"]
    if where == "device":
        import torch
        mates = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in mates]
        gaps = torch.from_numpy(h["gaps"].view(np.uint8).copy()).cuda()
    (lists, off), gl, pg, cg, idl = _four_stages(m, h, mates, gaps)
    print(where, want, gl, pg, idl)
    for name, st, count in (("gapped lists", gl, "fragments"), ("pileup", pg, "records"), ("indel calls", idl, "fragments")):
        assert {k: st[k] for k in SHARED} == want and st[count] == n, (name, st, want)
    assert cg["site_bases"] > 0 and cg["launches"] == 1 and pg["launches"] == 1
    # and the placements themselves are the checkers': the lists bit for bit, the aligned bases, the indel stage's events
    wl, wo, wst = h["lists"]
    if where == "device":
        lists, off = lists.cpu().numpy().view(rlib.MISMATCH_DTYPE).reshape(-1), off.cpu().numpy().view(np.uint64)
    assert np.array_equal(off, wo) and all(np.array_equal(lists[k][:int(wo[-1])], wl[k]) for k in ("off", "ref", "base"))
    assert gl["aligned_bases"] == pg["aligned_bases"] == wst["aligned_bases"] and gl["deleted"] == pg["deleted"] and gl["inserted"] == pg["inserted"]
    assert idl["ungapped"] == pg["ungapped"] and idl["events"] + idl["on_n"] + idl["low_qual"] == idl["placed"] - idl["ungapped"]
    m.close()


def _work(m, w):
    """a mapping quality fold, a gap rescue, a gapped pileup add and an indel add on the workload's few hundred fragments"""
    b1, b2 = w["b1"], w["b2"]
    hits, off = m.match_all(b1.bases, b1.qual, b1.offsets)
    m.mapq_hits(hits, off)
    pairs, s1, s2 = m.match_pairs_singles(b1, b2, w["min_ins"], w["max_ins"])
    gaps = m.gap_rescue(b1, b2, pairs, s1, s2, w["min_ins"], w["max_ins"], **w["prm"]._asdict())
    m.pileup_begin(MIN_QUAL)
    m.pileup_add_pairs(b1, b2, pairs)
    m.pileup_add_gapped(b1, b2, gaps)
    m.pileup_finish()
    m.indel_begin()
    m.indel_add(b1, b2, gaps)
    return gaps


def _four_stats(m):
    return m.mapq_stats(), m.gap_stats(), m.indel_stats(), m.pileup_gapped_stats()


def test_destroying_one_context_leaves_the_others_state_alone():
    wa, wb = gw.workload(seed=1, n=300), gw.workload(seed=2, n=200)
    ma, mb = _matcher(wa["g"].sym, wa["g"].frag_start, index=True), _matcher(wb["g"].sym, wb["g"].frag_start, index=True)
    _work(ma, wa)
    gaps = _work(mb, wb)
    before_a, before = _four_stats(ma), _four_stats(mb)
    mq, gp, idl, pg = before
    assert mq["launches"] > 0 and gp["unique"] > 20 and idl["placed"] + idl["invalid"] == pg["placed"] == gp["unique"] and idl["fragments"] == wb["b1"].n_reads, before
    assert before_a[1]["fragments"] == wa["b1"].n_reads != wb["b1"].n_reads
    ma.close()
    assert _four_stats(mb) == before, "the other context's four statistics"
    mb.indel_add(wb["b1"], wb["b2"], gaps)                              # a further add on it works
    after = mb.indel_stats()
    assert {k: after[k] for k in ("fragments", "placed", "events", "ungapped")} == {k: 2 * idl[k] for k in ("fragments", "placed", "events", "ungapped")}
    assert mb.indel_finish()[0] > 0 and mb.pileup_depth_gapped(0, wb["g"].n).any()
    fresh = _matcher(wa["g"].sym, wa["g"].frag_start)                   # (its address may be the destroyed context's)
    for name, st in zip(("mapq", "gap rescue", "indel calls", "gapped pileup"), _four_stats(fresh)):
        assert not any(st.values()), (name, st)
    fresh.close()
    mb.close()


def test_the_three_entry_points_refuse_as_before(hand):
    """codes and messages as the library answered before the entry points shared stage_gapped (REAL_HIP_E_INVALID and
    "invalid argument: <stage>: null gaps", "... the gap records must be 16-byte aligned", "... the two batches hold different
    numbers of reads"), nothing launched"""
    import torch
    h = hand
    b1, b2, gaps = h["b1"], h["b2"], h["gaps"]
    n = int(gaps.shape[0])
    m = _matcher(h["sym"], h["frag_start"])
    L, INV = m._L, rlib.REAL_HIP_E_INVALID
    err = lambda: L.real_hip_last_error(m._h).decode()      # noqa: E731
    said = lambda stage, what: "invalid argument: %s: %s" % (stage, what)      # noqa: E731
    m.pileup_begin(MIN_QUAL)                                 # the pileup's add may come now
    entries = [("pileup", lambda r1, r2, g: L.real_hip_pileup_add_gapped(m._h, C.byref(r1), C.byref(r2), g))]
    host_out = (np.zeros(16, dtype=rlib.MISMATCH_DTYPE), np.zeros(n + 1, dtype=np.uint64))
    dev_out = (torch.zeros(16, dtype=torch.int32, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda"))
    nout = C.c_uint64(0)

    def lists(r1, r2, g):
        out, off = dev_out if r1.on_device else host_out
        return L.real_hip_mismatches_gapped(m._h, C.byref(r1), C.byref(r2), g, _addr(out), 16, C.byref(nout), _addr(off))
    entries.append(("gapped mismatch lists", lists))
    dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)]
    dgaps = torch.from_numpy(np.concatenate([np.zeros(16, np.uint8), gaps.view(np.uint8)])).cuda()      # (16 bytes in front: the records start aligned)
    assert dgaps.data_ptr() % 16 == 0
    for turn in range(2):
        for stage, entry in entries:
            r1, r2, short = m._mate_batch(b1), m._mate_batch(b2), m._mate_batch(b2.part(0, 5))
            d1, d2 = m._mate_batch(dev[0]), m._mate_batch(dev[1])
            assert entry(r1, r2, None) == INV and err() == said(stage, "null gaps"), err()
            assert entry(d1, d2, None) == INV and err() == said(stage, "null gaps"), err()
            for shift in (4, 8):
                assert entry(d1, d2, dgaps.data_ptr() + 16 + shift) == INV and err() == said(stage, "the gap records must be 16-byte aligned"), err()
            assert entry(r1, short, gaps.ctypes.data) == INV and err() == said(stage, "the two batches hold different numbers of reads"), err()
        if turn == 0:
            # the indel add: its state comes first ("add without begin"), so it is asked on a finished pileup with the stage begun
            assert L.real_hip_indel_add(m._h, C.byref(m._mate_batch(b1)), C.byref(m._mate_batch(b2)), None) == INV and err() == said("indel calls", "add without begin")
            m.pileup_add_pairs(h["pb1"], h["pb2"], h["pairs"])
            m.pileup_finish()
            m.call_begin()
            m.indel_begin()
            entries = [("indel calls", lambda r1, r2, g: L.real_hip_indel_add(m._h, C.byref(r1), C.byref(r2), g)),
                       ("calls", lambda r1, r2, g: L.real_hip_call_add_gapped(m._h, C.byref(r1), C.byref(r2), g))]
    st = m.gapped_list_stats(), m.pileup_gapped_stats(), m.indel_stats()
    assert all(s["launches"] == 0 for s in st), st
    # and aligned device records behind the refusals are taken
    m.indel_add(dev[0], dev[1], dgaps[16:])
    m.call_add_gapped(dev[0], dev[1], dgaps[16:])
    assert m.indel_stats()["placed"] == h["want"]["placed"] and m.pileup_gapped_stats()["launches"] == 1
    m.close()


def _addr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data
