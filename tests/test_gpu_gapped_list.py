"""Gapped mismatch lists on the device (real_hip_mismatches_gapped) against the checker of gapped_list_checker.py: every entry bit
for bit, the offsets and every semantic counter -- on records that are real_hip_gap_rescue's own, and on records written by hand
(gapped_list_workloads.hand_cases: the lengths, splits, gap lengths, text edges, N bits and refused records the kernel takes
another path at)."""
import ctypes as C

import numpy as np
import pytest

import gap_checker as gc
import gap_workloads as gw
import gapped_list_checker as glc
import gapped_list_workloads as glw
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions

pytestmark = pytest.mark.gpu


def _matcher(sym, frag_start, fileid=0, index=False):
    m = PairMatcher(RealOptions(seedl=gw.SEEDL, seedkmax=2, totalkmax=gw.TOTALKMAX, scores=False, filter_level=0).normalise())
    m.set_text_symbols(fileid, sym, frag_start)
    if index:
        m.build_index_block()
    return m


def _counters(st):
    return {k: st[k] for k in glc.COUNTERS}


def _assert_lists(got, want, what):
    (gl, go), (wl, wo, _) = got, want
    assert np.array_equal(np.asarray(go, dtype=np.uint64), wo), what
    bad = np.nonzero(np.asarray(gl).view(np.uint32) != wl.view(np.uint32))[0]
    assert gl.shape == wl.shape and bad.size == 0, "%s: %d entries differ, first %d: got %r want %r" % (what, bad.size, bad[0], gl[bad[0]], wl[bad[0]])


_H = {}


def _hand():
    """the hand-made records and the checker's lists of them: computed once, never changed"""
    if not _H:
        h = glw.hand_cases()
        _H["h"] = h
        _H["want"] = glc.gapped_lists(h["sym"], 0, h["b1"], h["b2"], h["gaps"])
    return _H["h"], _H["want"]


def _room(want):
    """room for the whole list at once: a call that overflowed has counted, and the mirror's second call would count again"""
    return int(want[1][-1]) + 1


def _part(h, want, lo, hi):
    lists, off, _ = want
    sub = glc.gapped_lists(h["sym"], 0, h["b1"].part(lo, hi), h["b2"].part(lo, hi), h["gaps"][lo:hi])
    assert sub[0].tobytes() == lists[int(off[lo]):int(off[hi])].tobytes()        # (the checker's own halves rule)
    return sub


def test_hand_made_records_against_the_checker():
    h, want = _hand()
    m = _matcher(h["sym"], h["frag_start"])
    keep = h["gaps"].copy()
    got = m.mismatches_gapped(h["b1"], h["b2"], h["gaps"], cap=_room(want))
    _assert_lists(got, want, "hand-made records")
    st = m.gapped_list_stats(reset=True)
    print(st)
    assert _counters(st) == want[2] and st["launches"] == 3 and st["kernel_ms"] > 0, (st, want[2])
    assert keep.tobytes() == h["gaps"].tobytes(), "the records are inputs"
    assert want[2]["invalid"] >= 11 and want[2]["other_file"] == 1 and want[2]["on_n"] > 0 and want[2]["disagree"] > 0
    # the refused records gave empty lists and the call succeeded; the fitting record behind them is listed
    off = got[1]
    for i, note in enumerate(h["what"]):
        if note in glw.EMPTY_NOTES:
            assert off[i + 1] == off[i], note
    assert off[-1] > off[-2]
    assert _counters(m.gapped_list_stats()) == dict.fromkeys(glc.COUNTERS, 0)
    m.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(n):
    h, want = _hand()
    m = _matcher(h["sym"], h["frag_start"])
    lo = 40 - n // 8
    sub = _part(h, want, lo, lo + n)
    got = m.mismatches_gapped(h["b1"].part(lo, lo + n), h["b2"].part(lo, lo + n), h["gaps"][lo:lo + n], cap=_room(sub))
    _assert_lists(got, sub, "n_reads %d" % n)
    assert _counters(m.gapped_list_stats(reset=True)) == sub[2]
    m.close()


def test_halves_device_arrays_and_packed_batches():
    import torch
    h, want = _hand()
    b1, b2, gaps = h["b1"], h["b2"], h["gaps"]
    n_all = b1.n_reads
    m = _matcher(h["sym"], h["frag_start"])
    half = n_all // 2 + 1
    parts = [m.mismatches_gapped(b1.part(a, b), b2.part(a, b), gaps[a:b], cap=_room(want)) for a, b in ((0, half), (half, n_all))]
    lists = np.concatenate([p[0] for p in parts])
    off = np.concatenate([parts[0][1], parts[1][1][1:] + parts[0][1][-1]])
    _assert_lists((lists, off), want, "two halves")
    assert _counters(m.gapped_list_stats(reset=True)) == want[2]
    # device reads and records (on_device = 1): device outputs; then device reads with host records (on_device = 2)
    dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)]
    dgaps = torch.from_numpy(gaps.view(np.uint8).copy()).cuda()
    dl, do = m.mismatches_gapped(dev[0], dev[1], dgaps, cap=_room(want))
    _assert_lists((dl.cpu().numpy().view(rlib.MISMATCH_DTYPE), do.cpu().numpy().view(np.uint64)), want, "device arrays")
    assert _counters(m.gapped_list_stats(reset=True)) == want[2]
    _assert_lists(m.mismatches_gapped(dev[0], dev[1], gaps), want, "device reads, host records")
    m.gapped_list_stats(reset=True)
    # packed batches whose reads start inside a byte
    keep, bb = [], []
    for b in (b1, b2):
        packed = synth.pack_bases(np.concatenate([np.zeros(1, np.uint8), b.bases]))
        flags, offs = synth.read_nflags(b.bases, b.offsets), (b.offsets + np.uint64(1)).astype(np.uint64)
        bb.append(rlib.sized(rlib.RealHipBatch, on_device=0, n_reads=b.n_reads, bases=packed.ctypes.data, qual=None, offsets=offs.ctypes.data, packed=1,
                             nflags=flags.ctypes.data))
        keep += [packed, flags, offs]
    total = int(want[1][-1])
    out, moff, n_out = np.zeros(total, dtype=rlib.MISMATCH_DTYPE), np.zeros(n_all + 1, dtype=np.uint64), C.c_uint64(0)
    m._check(m._L.real_hip_mismatches_gapped(m._h, C.byref(bb[0]), C.byref(bb[1]), gaps.ctypes.data, out.ctypes.data, total, C.byref(n_out), moff.ctypes.data))
    assert n_out.value == total
    _assert_lists((out, moff), want, "packed, reads start inside a byte")
    assert _counters(m.gapped_list_stats(reset=True)) == want[2]
    m.close()


def test_two_genome_files():
    """the same records against file 1: those of file 0 are another file's, the one of file 1 is listed"""
    h, want = _hand()
    m = _matcher(h["sym"], h["frag_start"], fileid=1)
    w1 = glc.gapped_lists(h["sym"], 1, h["b1"], h["b2"], h["gaps"])
    got = m.mismatches_gapped(h["b1"], h["b2"], h["gaps"], cap=_room(w1))
    _assert_lists(got, w1, "file 1")
    assert _counters(m.gapped_list_stats(reset=True)) == w1[2] and w1[2]["placed"] == 1 and w1[2]["other_file"] == want[2]["placed"] + want[2]["invalid"]
    # a text of its own as file 1, the records half and half
    g2 = np.roll(h["sym"], 977)
    gaps = h["gaps"].copy()
    gaps["fileid"][::2] = 1
    m.set_text_symbols(1, g2, h["frag_start"])
    w2 = glc.gapped_lists(g2, 1, h["b1"], h["b2"], gaps)
    _assert_lists(m.mismatches_gapped(h["b1"], h["b2"], gaps, cap=_room(w2)), w2, "mixed records, file 1")
    assert _counters(m.gapped_list_stats(reset=True)) == w2[2] and w2[2]["placed"] > 100 and w2[2]["other_file"] > 100
    m.close()


def test_overflow_protocol_empty_batch_and_loud_errors():
    h, want = _hand()
    b1, b2, gaps = h["b1"], h["b2"], h["gaps"]
    n, total = b1.n_reads, int(want[1][-1])
    m = _matcher(h["sym"], h["frag_start"])
    r1, r2 = m._mate_batch(b1), m._mate_batch(b2)
    out, moff, n_out = np.full(total, 0xAB, dtype=np.uint8).repeat(4).view(rlib.MISMATCH_DTYPE), np.zeros(n + 1, dtype=np.uint64), C.c_uint64(0)
    call = lambda *a: m._L.real_hip_mismatches_gapped(m._h, *a)             # noqa: E731
    # one short of the total: E_OVERFLOW, nothing written to out, the offsets and the total written
    assert call(C.byref(r1), C.byref(r2), gaps.ctypes.data, out.ctypes.data, total - 1, C.byref(n_out), moff.ctypes.data) == rlib.REAL_HIP_E_OVERFLOW
    assert n_out.value == total and np.array_equal(moff, want[1]) and (out.view(np.uint8) == 0xAB).all()
    st = m.gapped_list_stats(reset=True)
    assert _counters(st) == want[2] and st["launches"] == 2                  # (counted, not emitted)
    # the mirror grows once
    _assert_lists(m.mismatches_gapped(b1, b2, gaps, cap=1), want, "grown from cap 1")
    m.gapped_list_stats(reset=True)
    # n_reads = 0
    e1, e2 = m._mate_batch(b1.part(0, 0)), m._mate_batch(b2.part(0, 0))
    moff[:] = 7
    assert call(C.byref(e1), C.byref(e2), None, None, 0, C.byref(n_out), moff.ctypes.data) == rlib.REAL_HIP_OK and n_out.value == 0 and moff[0] == 0
    lists, off = m.mismatches_gapped(b1.part(0, 0), b2.part(0, 0), gaps[:0])
    assert lists.shape[0] == 0 and off.tolist() == [0]
    # the error returns: nothing launched
    launches = m.gapped_list_stats()["launches"]
    args = [C.byref(r1), C.byref(r2), gaps.ctypes.data, out.ctypes.data, total, C.byref(n_out), moff.ctypes.data]
    for k in (0, 1, 2, 3, 5, 6):
        assert call(*[None if j == k else a for j, a in enumerate(args)]) == rlib.REAL_HIP_E_INVALID, k
    assert "gapped mismatch lists" in m._L.real_hip_last_error(m._h).decode()
    short = m._mate_batch(b2.part(0, 5))
    assert call(*(args[:1] + [C.byref(short)] + args[2:])) == rlib.REAL_HIP_E_INVALID and "different numbers" in m._L.real_hip_last_error(m._h).decode()
    st = rlib.sized(rlib.RealHipGappedListStats)
    st.struct_size += 8
    assert m._L.real_hip_gapped_list_stats_get(m._h, C.byref(st), 0) == rlib.REAL_HIP_E_INVALID
    assert (out.view(np.uint8) == 0xAB).all() and m.gapped_list_stats()["launches"] == launches, "nothing was launched"
    assert call(*args) == rlib.REAL_HIP_OK
    _assert_lists((out, moff), want, "after the errors")
    m.close()
    bare = PairMatcher(RealOptions(seedl=gw.SEEDL, seedkmax=2, totalkmax=gw.TOTALKMAX, scores=False, filter_level=0).normalise())
    with pytest.raises(rlib.RealHipError) as e:
        bare.mismatches_gapped(b1, b2, gaps)
    assert e.value.status == rlib.REAL_HIP_E_STATE
    bare.close()


# the rescue's own records: the shortest read it takes at flank 8 / gap 8, the word boundaries, the longest read
@pytest.mark.parametrize("patl", [25, 33, 64, 100, 320])
def test_records_of_the_gap_rescue(patl):
    long = patl > 200
    w = glw.workload(seed=patl, patl=patl, min_ins=300 if long else gw.MIN_INS, max_ins=600 if long else gw.MAX_INS, n=120 if long else 250,
                     size=200_000 if long else 100_000, per_class=4 if long else gw.PER_CLASS)
    g = w["g"]
    m = _matcher(g.sym, g.frag_start, index=True)
    pairs, s1, s2 = m.match_pairs_singles(w["b1"], w["b2"], w["min_ins"], w["max_ins"])
    gaps = m.gap_rescue(w["b1"], w["b2"], pairs, s1, s2, w["min_ins"], w["max_ins"], **w["prm"]._asdict())
    rec = np.zeros(gaps.shape[0], dtype=gc.REC_DTYPE)
    for k in gc.REC_DTYPE.names:
        rec[k] = gaps[k]
    want = glc.gapped_lists(g.sym, 0, w["b1"], w["b2"], rec)
    got = m.mismatches_gapped(w["b1"], w["b2"], gaps, cap=_room(want))
    _assert_lists(got, want, "patl %d" % patl)
    st = m.gapped_list_stats(reset=True)
    print(patl, st)
    assert _counters(st) == want[2] and st["disagree"] == 0 and st["on_n"] == 0 and st["invalid"] == 0 and st["other_file"] == 0
    assert st["placed"] == m.gap_stats()["unique"] >= 10 and st["deleted"] > 0 and st["inserted"] > 0
    m.close()
