"""Mate search on the device (real_hip_match_pairs_search / real_hip_pair_search) against the brute-force checker of
mate_search_checker.py: every field of every record and both FP64 values bit for bit, the four counters exactly."""
import ctypes as C

import numpy as np
import pytest

import mate_search_checker as mc
import mate_search_hand as mh
import mate_search_workloads as mw
import pairs_checker as pc
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions

pytestmark = pytest.mark.gpu

# scores, totalkmax, filter_level, table_kind, prefix_bits, seedl, ragged, (patl1, patl2)
CASES = [(1, 3, 2, 0, 0, 32, False, (100, 100)),
         (0, 3, 0, 2, 29, 32, False, (100, 80)),
         (0, 5, 2, 3, 13, 16, True, (100, 80)),
         (1, 5, 2, 3, 13, 16, True, (100, 100))]


def _opts(seedl, totalkmax, scores, filter_level):
    return RealOptions(seedl=seedl, seedkmax=2, totalkmax=totalkmax, scores=bool(scores), filter_level=filter_level).normalise()


def _matcher(g, seedl, tk, scores, fl, pb=0, tkind=0, fileid=0, index=True):
    m = PairMatcher(_opts(seedl, tk, scores, fl), prefix_bits=pb, table_kind=tkind)
    m.set_text_symbols(fileid, g.sym, g.frag_start)
    if index:
        m.build_index_block()
    return m


def _counters(st):
    return {k: st[k] for k in mc.COUNTERS}


def _product_hits(h):
    """hits in the oracle's layout -> real_hip_hit records"""
    out = np.zeros(h.shape[0], dtype=rlib.HIT_DTYPE)
    for k in ("pos", "score", "frag", "k", "inverted"):
        out[k] = h[k]
    return out


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", ["iid", "families"])
def test_match_pairs_search_against_the_checker(ora, kind, case):
    scores, tk, fl, tkind, pb, seedl, ragged, patl = case
    g, b1, b2, _ = mw.search_workload(kind, ragged, patl, seedl, tk)
    f = mw.oracle_lists(ora, g, b1, b2, seedl, tk, scores, fl)
    args = (b1, b2, mw.MIN_INS, mw.MAX_INS, scores, ora.filter_mult(fl, tk), seedl, tk)
    off, _ = mc.check_pairs_search(ora, {0: g}, [f], *args, search=False)
    on, ctr = mc.check_pairs_search(ora, {0: g}, [f], *args)
    mw.assert_coverage(off, on, f, "%s %r" % (kind, case))
    m = _matcher(g, seedl, tk, scores, fl, pb, tkind)
    assert m.table_kind == {0: rlib.LAYOUT_STARTS, 2: rlib.LAYOUT_DIGEST, 3: rlib.LAYOUT_ROWS}[tkind], m.table_kind
    got = m.match_pairs(b1, b2, mw.MIN_INS, mw.MAX_INS, mate_search=True)
    pc.assert_records_equal(got, on, "search on %s %r" % (kind, case))
    st = m.mate_search_stats(reset=True)
    assert _counters(st) == ctr and st["fragments"] == b1.n_reads and st["launches"] == 1 and st["kernel_ms"] > 0, (st, ctr)
    # search off: the records of real_hip_match_pairs are what they were, and nothing is counted
    pc.assert_records_equal(m.match_pairs(b1, b2, mw.MIN_INS, mw.MAX_INS), off, "search off")
    assert m.mate_search_stats()["fragments"] == 0
    # a max_anchors that bites
    cap = 1 if kind == "iid" else 4
    on_cap, ctr_cap = mc.check_pairs_search(ora, {0: g}, [f], *args, max_anchors=cap)
    assert ctr_cap["anchors_skipped"] > 0 and (on_cap["state"] != on["state"]).any()
    pc.assert_records_equal(m.match_pairs(b1, b2, mw.MIN_INS, mw.MAX_INS, mate_search=True, max_anchors=cap), on_cap, "max_anchors %d" % cap)
    assert _counters(m.mate_search_stats(reset=True)) == ctr_cap
    # the join and the search as two calls on the matcher's own hit lists (host arrays) = the one call
    h1, o1 = m.match_all(b1.bases, b1.qual, b1.offsets)
    h2, o2 = m.match_all(b2.bases, b2.qual, b2.offsets)
    rec = m.pair_hits(h1, o1, mw.lens_of(b1), h2, o2, mw.lens_of(b2), mw.MIN_INS, mw.MAX_INS)
    pc.assert_records_equal(rec, off, "pair_hits")
    rec = m.pair_search(b1, b2, h1, o1, h2, o2, mw.MIN_INS, mw.MAX_INS, pairs=rec)
    pc.assert_records_equal(rec, on, "pair_hits + pair_search")
    assert _counters(m.mate_search_stats(reset=True)) == ctr
    m.close()


def test_device_inputs_and_batch_forms(ora):
    """device batches and records; 2-bit packed bases with nflags, no qualities, uniform lengths"""
    import torch
    scores, tk, fl, seedl = 1, 3, 2, 32
    g, b1, b2, _ = mw.search_workload("iid", False, (100, 80), seedl, tk)
    f = mw.oracle_lists(ora, g, b1, b2, seedl, tk, scores, fl)
    args = (mw.MIN_INS, mw.MAX_INS, scores, ora.filter_mult(fl, tk), seedl, tk)
    on, ctr = mc.check_pairs_search(ora, {0: g}, [f], b1, b2, *args)
    m = _matcher(g, seedl, tk, scores, fl)
    dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)]
    rec = torch.zeros(b1.n_reads * 40, dtype=torch.uint8, device="cuda")
    m.match_pairs(dev[0], dev[1], mw.MIN_INS, mw.MAX_INS, pairs=rec, fresh=True, mate_search=True)
    pc.assert_records_equal(rec.cpu().numpy().view(rlib.PAIR_DTYPE), on, "device batches")
    assert _counters(m.mate_search_stats(reset=True)) == ctr
    # device anchors through real_hip_pair_search, on top of the join's records
    h1, o1 = m.match_all(b1.bases, b1.qual, b1.offsets)
    h2, o2 = m.match_all(b2.bases, b2.qual, b2.offsets)
    d = [torch.from_numpy(x.view(np.int32).reshape(-1, 4).copy()).cuda() if x.dtype == rlib.HIT_DTYPE else torch.from_numpy(x.view(np.int64).copy()).cuda()
         for x in (h1, o1, h2, o2)]
    rec2 = torch.from_numpy(m.pair_hits(h1, o1, mw.lens_of(b1), h2, o2, mw.lens_of(b2), mw.MIN_INS, mw.MAX_INS).view(np.uint8).copy()).cuda()
    m.pair_search(dev[0], dev[1], *d, mw.MIN_INS, mw.MAX_INS, pairs=rec2)
    pc.assert_records_equal(rec2.cpu().numpy().view(rlib.PAIR_DTYPE), on, "device anchors")
    # packed, nflags, qual == NULL, uniform length (offsets == NULL): the oracle sees reads without qualities
    n1 = synth.ReadBatch(bases=b1.bases, qual=None, offsets=b1.offsets, ids=b1.ids)
    n2 = synth.ReadBatch(bases=b2.bases, qual=None, offsets=b2.offsets, ids=b2.ids)
    fq = mw.oracle_lists(ora, g, n1, n2, seedl, tk, scores, fl)
    on_q, ctr_q = mc.check_pairs_search(ora, {0: g}, [fq], n1, n2, *args)
    m.mate_search_stats(reset=True)
    keep, bb = [], []
    for b, patl in ((b1, 100), (b2, 80)):
        packed, flags = synth.pack_bases(b.bases), synth.read_nflags(b.bases, b.offsets)
        rb = rlib.RealHipBatch()
        rb.struct_size, rb.on_device, rb.n_reads = C.sizeof(rlib.RealHipBatch), 0, b.n_reads
        rb.bases, rb.qual, rb.offsets, rb.patl, rb.packed, rb.nflags, rb.fresh = packed.ctypes.data, None, None, patl, 1, flags.ctypes.data, 1
        keep += [packed, flags]
        bb.append(rb)
    out = PairMatcher.new_pair_info(b1.n_reads)
    pp, sp = m._pair_params(mw.MIN_INS, mw.MAX_INS), m._search_params(0)
    m._check(m._L.real_hip_match_pairs_search(m._h, C.byref(bb[0]), C.byref(bb[1]), C.byref(pp), C.byref(sp), out.ctypes.data))
    pc.assert_records_equal(out, on_q, "packed, no qualities, uniform length")
    assert _counters(m.mate_search_stats(reset=True)) == ctr_q
    # a packed batch whose reads start inside a byte: one base in front of everything, offsets shifted by it
    bb = []
    for b in (b1, b2):
        packed = synth.pack_bases(np.concatenate([np.zeros(1, np.uint8), b.bases]))
        flags, offs = synth.read_nflags(b.bases, b.offsets), (b.offsets + np.uint64(1)).astype(np.uint64)
        rb = rlib.RealHipBatch()
        rb.struct_size, rb.on_device, rb.n_reads = C.sizeof(rlib.RealHipBatch), 0, b.n_reads
        rb.bases, rb.qual, rb.offsets, rb.packed, rb.nflags, rb.fresh = packed.ctypes.data, None, offs.ctypes.data, 1, flags.ctypes.data, 1
        keep += [packed, flags, offs]
        bb.append(rb)
    out = PairMatcher.new_pair_info(b1.n_reads)
    m._check(m._L.real_hip_match_pairs_search(m._h, C.byref(bb[0]), C.byref(bb[1]), C.byref(pp), C.byref(sp), out.ctypes.data))
    pc.assert_records_equal(out, on_q, "packed, reads start inside a byte")
    m.close()


@pytest.mark.parametrize("scores", [1, 0])
def test_two_genome_files_fold_in_both_orders(ora, scores):
    seedl, tk, fl = 32, 3, 2
    g0, a1, a2, _ = mw.search_workload("iid", False, (100, 80), seedl, tk, n=400, seed=31, size=200_000)
    g1, c1, c2, _ = mw.search_workload("families", False, (100, 80), seedl, tk, n=300, seed=32, size=250_000)
    g1.sym[1000:2600] = g0.sym[1000:2600]                            # a stretch both files hold
    b1, b2 = synth.concat_batches([a1, c1]), synth.concat_batches([a2, c2])
    m = PairMatcher(_opts(seedl, tk, scores, fl))
    recs = {}
    for order in ((0, 1), (1, 0)):
        rec = None
        for fid in order:
            g = (g0, g1)[fid]
            m.set_text_symbols(fid, g.sym, g.frag_start)
            m.build_index_block()
            rec = m.match_pairs(b1, b2, mw.MIN_INS, mw.MAX_INS, pairs=rec, mate_search=True)
        recs[order] = rec
    files = [mw.oracle_lists(ora, g, b1, b2, seedl, tk, scores, fl, fileid=fid) for fid, g in enumerate((g0, g1))]
    want, _ = mc.check_pairs_search(ora, {0: g0, 1: g1}, files, b1, b2, mw.MIN_INS, mw.MAX_INS, scores, ora.filter_mult(fl, tk), seedl, tk)
    pc.assert_records_equal(recs[(0, 1)], want, "files 0, 1")
    pc.assert_records_equal(recs[(1, 0)], want, "files 1, 0")
    uniq = want["state"] == pc.UNIQUE
    assert (uniq & (want["fileid"] == 0)).sum() > 50 and (uniq & (want["fileid"] == 1)).sum() > 50
    m.close()


# ---- hand-made anchors through real_hip_pair_search ---------------------------------------------------------------------
MIN_H, MAX_H, L1, L2 = mh.MIN_H, mh.MAX_H, mh.L1, mh.L2


@pytest.mark.parametrize("scores", [1, 0])
def test_pair_search_on_hand_made_anchors(ora, scores):
    tk, seedl, fl = 3, 32, 2
    g = mh.classic_genome()
    S = mc.Searcher(ora, g, seedl, tk, scores, MIN_H, MAX_H)
    F = mh.classic_cases(g, S, tk)
    b1, b2, (h1, o1), (h2, o2) = mh.batches(F)
    fm = ora.filter_mult(fl, tk)
    want, ctr = mc.search_only(ora, {0: g}, [(0, h1, o1, h2, o2)], b1, b2, MIN_H, MAX_H, scores, fm, seedl, tk)
    assert [int(s) for s in want["state"]] == [f[5] for f in F], [(f[0], int(s)) for f, s in zip(F, want["state"]) if int(s) != f[5]]
    m = _matcher(g, seedl, tk, scores, fl, index=False)             # the search needs the text, not the index
    p1, p2 = _product_hits(h1), _product_hits(h2)
    got = m.pair_search(b1, b2, p1, o1, p2, o2, MIN_H, MAX_H)
    pc.assert_records_equal(got, want, "hand-made anchors")
    st = m.mate_search_stats(reset=True)
    assert _counters(st) == ctr and ctr["placements"] == sum(len(f[3]) + len(f[4]) for f in F if f[5] == pc.UNIQUE), (st, ctr)
    # a placement that is also a hit: the record of the join does not change
    i = [f[0] for f in F].index("both mates anchor: one location")
    lens = (mw.lens_of(b1), mw.lens_of(b2))
    rec = m.pair_hits(p1, o1, lens[0], p2, o2, lens[1], MIN_H, MAX_H)
    assert rec["state"][i] == pc.UNIQUE
    again = m.pair_search(b1, b2, p1, o1, p2, o2, MIN_H, MAX_H, pairs=rec.copy())
    pc.assert_records_equal(again[i:i + 1], rec[i:i + 1], "a placement that is also a hit")
    pc.assert_records_equal(again, np.array([pc.merge(rec[j], want[j], pc.eps_of(scores, fm, L1, L2)) for j in range(len(F))]), "in/out records")
    # max_insert at the stated limit runs (and equals the checker), one above is refused, like a read of 321 bases and bad structs
    lim = rlib.REAL_HIP_MATE_SEARCH_MAX_INSERT
    wide, _ = mc.search_only(ora, {0: g}, [(0, h1, o1, h2, o2)], b1, b2, MIN_H, lim, scores, fm, seedl, tk)
    pc.assert_records_equal(m.pair_search(b1, b2, p1, o1, p2, o2, MIN_H, lim), wide, "max_insert at the limit")
    assert (wide["state"] != want["state"]).any()
    m.mate_search_stats(reset=True)
    with pytest.raises(rlib.RealHipError) as e:
        m.pair_search(b1, b2, p1, o1, p2, o2, MIN_H, lim + 1)
    assert e.value.status == rlib.REAL_HIP_E_UNSUPPORTED
    long1 = synth.ReadBatch(bases=np.zeros(321, np.uint8), qual=np.full(321, 30, np.uint8), offsets=np.array([0, 321], np.uint64), ids=None)
    short2 = synth.ReadBatch(bases=np.zeros(80, np.uint8), qual=np.full(80, 30, np.uint8), offsets=np.array([0, 80], np.uint64), ids=None)
    none = (np.zeros(0, rlib.HIT_DTYPE), np.zeros(2, np.uint64))
    with pytest.raises(rlib.RealHipError) as e:
        m.pair_search(long1, short2, *none, *none, MIN_H, MAX_H)
    assert e.value.status == rlib.REAL_HIP_E_UNSUPPORTED
    pp, sp = m._pair_params(MIN_H, MAX_H), m._search_params(0)
    sp.struct_size -= 4
    bb1, bb2 = m._mate_batch(b1), m._mate_batch(b2)
    out = PairMatcher.new_pair_info(len(F))
    ptrs = (p1.ctypes.data, o1.ctypes.data, p2.ctypes.data, o2.ctypes.data)
    assert m._L.real_hip_pair_search(m._h, C.byref(pp), C.byref(sp), C.byref(bb1), C.byref(bb2), *ptrs, 0, 1, out.ctypes.data) == rlib.REAL_HIP_E_INVALID
    assert m._L.real_hip_pair_search(m._h, C.byref(pp), None, C.byref(bb1), C.byref(bb2), *ptrs, 0, 1, out.ctypes.data) == rlib.REAL_HIP_E_INVALID
    assert m._L.real_hip_match_pairs_search(m._h, C.byref(bb1), C.byref(bb2), C.byref(pp), C.byref(sp), out.ctypes.data) == rlib.REAL_HIP_E_INVALID
    assert m.mate_search_stats()["launches"] == 0, "nothing was launched by the refused calls"
    with pytest.raises(rlib.RealHipError) as e:                     # the one call needs the index
        m.match_pairs(b1, b2, MIN_H, MAX_H, mate_search=True)
    assert e.value.status == rlib.REAL_HIP_E_STATE
    m.build_index_block()
    with pytest.raises(rlib.RealHipError) as e:
        m.match_pairs(long1, short2, MIN_H, MAX_H, mate_search=True)
    assert e.value.status == rlib.REAL_HIP_E_UNSUPPORTED
    assert m.match_pairs(long1, short2, MIN_H, MAX_H).shape[0] == 1   # (without the search such a read is matched as before)
    m.close()
