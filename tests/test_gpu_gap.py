"""Gap rescue on the device (real_hip_gap_rescue) against the checker of gap_checker.py: every field of every record and every
semantic counter, on records that are the unchanged output of real_hip_match_pairs_singles for the same reads."""
import ctypes as C

import numpy as np
import pytest

import gap_checker as gc
import gap_workloads as gw
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions, new_gap_place

pytestmark = pytest.mark.gpu


def _matcher(g, fileid=0, index=True):
    m = PairMatcher(RealOptions(seedl=gw.SEEDL, seedkmax=2, totalkmax=gw.TOTALKMAX, scores=False, filter_level=0).normalise())
    m.set_text_symbols(fileid, g.sym, g.frag_start)
    if index:
        m.build_index_block()
    return m


def _kw(prm):
    return prm._asdict()


def _matched(w):
    """the matcher with the workload's text resident, and the records real_hip_match_pairs_singles leaves"""
    m = _matcher(w["g"], w["fileid"])
    pairs, s1, s2 = m.match_pairs_singles(w["b1"], w["b2"], w["min_ins"], w["max_ins"])
    return m, pairs, s1, s2


def _expected(w, pairs, s1, s2, out=None, g=None, fileid=None):
    t = gc.Text((g or w["g"]).sym, (g or w["g"]).frag_start, w["fileid"] if fileid is None else fileid)
    return gc.check_gap(t, w["b1"], w["b2"], pairs, s1, s2, w["min_ins"], w["max_ins"], w["prm"], out=out)


def _counters(st):
    return {k: st[k] for k in gc.COUNTERS}


def _check(w, what):
    m, pairs, s1, s2 = _matched(w)
    want, ctr = _expected(w, pairs, s1, s2)
    keep = (pairs.copy(), s1.copy(), s2.copy())
    got = m.gap_rescue(w["b1"], w["b2"], pairs, s1, s2, w["min_ins"], w["max_ins"], **_kw(w["prm"]))
    print(what, ctr)
    gc.assert_records_equal(got, want, what)
    st = m.gap_stats(reset=True)
    assert _counters(st) == ctr and st["launches"] == 2 and st["kernel_ms"] > 0, (st, ctr)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(keep, (pairs, s1, s2))), "the records are inputs"
    return m, pairs, s1, s2, want, ctr


_W = {}


def _workload(**kw):
    key = tuple(sorted((k, tuple(v) if isinstance(v, tuple) else v) for k, v in kw.items()))
    if key not in _W:
        _W[key] = gw.workload(**kw)
    return _W[key]


# the shortest read searched (2 * min_flank + max_gap + 1), the word boundaries, the longest read, and one the stage skips
@pytest.mark.parametrize("patl", [25, 32, 33, 64, 65, 100, 320, 321])
def test_read_lengths_against_the_checker(patl):
    long = patl > 200
    w = _workload(seed=patl, patl=patl, min_ins=300 if long else gw.MIN_INS, max_ins=600 if long else gw.MAX_INS, n=120 if long else 250,
                  size=200_000 if long else 100_000, per_class=4 if long else gw.PER_CLASS)
    m, _, _, _, want, ctr = _check(w, "patl %d" % patl)
    if patl == 321:
        assert ctr["skipped"] >= len(w["plants"]) and ctr["placed"] < ctr["eligible"]
    else:
        assert ctr["gapped"] >= 5 and ctr["unique"] >= 10, ctr
        assert long or {int(x) for x in gc.state_of(want["tag"])} == {0, 1, 2}
    m.close()


@pytest.mark.parametrize("max_gap,margin", [(1, 0), (16, 0), (8, 3)])
def test_gap_lengths_and_margin_against_the_checker(max_gap, margin):
    w = _workload(seed=7, prm=gc.default_params(gw.TOTALKMAX, max_gap=max_gap, margin=margin), max_ins=gw.MAX_INS + 2 * max_gap)
    m, _, _, _, want, ctr = _check(w, "max_gap %d margin %d" % (max_gap, margin))
    assert ctr["gapped"] >= 10 and int(np.abs(want["gap"].astype(int)).max()) == max_gap
    m.close()


# the number of concordant starts, set through the insert bounds: with max_gap on either side the examined starts end just
# below, at and just above one tile of 64 lanes and two
@pytest.mark.parametrize("width", [1, 63, 64, 65, 64 - 2 * 8 - 1, 64 - 2 * 8 + 1])
def test_window_widths_against_the_checker(width):
    w = _workload(seed=3, min_ins=260, max_ins=260 + width - 1, frag_l=260, n=150)
    m, _, _, _, want, ctr = _check(w, "window of %d starts" % width)
    assert ctr["gapped"] >= 8 and ctr["positions"] <= (ctr["eligible"] - ctr["skipped"]) * (width + 16)
    m.close()


def test_batch_sizes_halves_and_where_the_arrays_live():
    import torch
    w = _workload()
    m, pairs, s1, s2, want, ctr = _check(w, "whole")
    n_all = w["b1"].n_reads
    kw = _kw(w["prm"])
    for n in (0, 1, 65, 300):
        lo = max(0, min(n_all - n, 40 - n // 2))                          # (planted fragments inside)
        b1, b2 = w["b1"].part(lo, lo + n), w["b2"].part(lo, lo + n)
        got = m.gap_rescue(b1, b2, pairs[lo:lo + n], s1[lo:lo + n], s2[lo:lo + n], w["min_ins"], w["max_ins"], **kw)
        gc.assert_records_equal(got, want[lo:lo + n], "n_reads %d" % n)
        assert m.gap_stats(reset=True)["fragments"] == min(n, n_all)
    half = n_all // 2 + 1
    parts = [m.gap_rescue(w["b1"].part(a, b), w["b2"].part(a, b), pairs[a:b], s1[a:b], s2[a:b], w["min_ins"], w["max_ins"], **kw)
             for a, b in ((0, half), (half, n_all))]
    gc.assert_records_equal(np.concatenate(parts), want, "two halves")
    assert _counters(m.gap_stats(reset=True)) == ctr
    # device reads and records (on_device = 1), then device reads with host records (on_device = 2)
    dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (w["b1"], w["b2"])]
    drec = [torch.from_numpy(x.view(np.uint8).copy()).cuda() for x in (pairs, s1, s2)]
    out = torch.full((n_all * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    m.gap_rescue(dev[0], dev[1], *drec, w["min_ins"], w["max_ins"], out=out, fresh=True, **kw)
    gc.assert_records_equal(out.cpu().numpy().view(rlib.GAP_PLACE_DTYPE), want, "device arrays")
    assert _counters(m.gap_stats(reset=True)) == ctr
    got = m.gap_rescue(dev[0], dev[1], pairs, s1, s2, w["min_ins"], w["max_ins"], **kw)
    gc.assert_records_equal(got, want, "device reads, host records")
    m.close()


def test_packed_batches_with_a_read_starting_inside_a_byte():
    w = _workload()
    m, pairs, s1, s2, want, ctr = _check(w, "bytes")
    keep, bb = [], []
    for b in (w["b1"], w["b2"]):
        packed = synth.pack_bases(np.concatenate([np.zeros(1, np.uint8), b.bases]))      # one base in front of everything
        flags, offs = synth.read_nflags(b.bases, b.offsets), (b.offsets + np.uint64(1)).astype(np.uint64)
        rb = rlib.sized(rlib.RealHipBatch, on_device=0, n_reads=b.n_reads, bases=packed.ctypes.data, qual=None, offsets=offs.ctypes.data, packed=1,
                        nflags=flags.ctypes.data)
        keep += [packed, flags, offs]
        bb.append(rb)
    out = new_gap_place(w["b1"].n_reads)
    out["pos"] = 77                                                      # (fresh: output only)
    pp, gp = m._pair_params(w["min_ins"], w["max_ins"]), m._gap_params(**_kw(w["prm"]))
    m._check(m._L.real_hip_gap_rescue(m._h, C.byref(pp), C.byref(gp), C.byref(bb[0]), C.byref(bb[1]), pairs.ctypes.data, s1.ctypes.data,
                                      s2.ctypes.data, 1, out.ctypes.data))
    gc.assert_records_equal(out, want, "packed, reads start inside a byte")
    assert _counters(m.gap_stats(reset=True)) == ctr
    m.close()


def test_two_genome_files_fold_into_one_array():
    wa, wb = _workload(seed=1, n=100), _workload(seed=2, n=100, fileid=1)
    both = dict(wa, b1=gw.Batch([wa["b1"].read(i) for i in range(wa["b1"].n_reads)] + [wb["b1"].read(i) for i in range(wb["b1"].n_reads)]),
                b2=gw.Batch([wa["b2"].read(i) for i in range(wa["b2"].n_reads)] + [wb["b2"].read(i) for i in range(wb["b2"].n_reads)]))
    m = _matcher(wa["g"], 0)
    rec = m.match_pairs_singles(both["b1"], both["b2"], both["min_ins"], both["max_ins"])
    m.set_text_symbols(1, wb["g"].sym, wb["g"].frag_start)
    m.build_index_block()
    pairs, s1, s2 = m.match_pairs_singles(both["b1"], both["b2"], both["min_ins"], both["max_ins"], *rec)
    kw = _kw(both["prm"])
    # file 1 is resident: it goes first and starts the array; then file 0 folds into it (the text alone, no index)
    want1, ctr1 = _expected(both, pairs, s1, s2, g=wb["g"], fileid=1)
    got = m.gap_rescue(both["b1"], both["b2"], pairs, s1, s2, both["min_ins"], both["max_ins"], **kw)
    gc.assert_records_equal(got, want1, "file 1")
    assert _counters(m.gap_stats(reset=True)) == ctr1 and ctr1["other_file"] >= 20 and ctr1["placed"] >= 20, ctr1
    m.close()
    m = _matcher(wa["g"], 0, index=False)
    want, ctr0 = _expected(both, pairs, s1, s2, out=want1, g=wa["g"], fileid=0)
    got = m.gap_rescue(both["b1"], both["b2"], pairs, s1, s2, both["min_ins"], both["max_ins"], out=got, **kw)
    gc.assert_records_equal(got, want, "file 0 folded into file 1's records")
    assert _counters(m.gap_stats(reset=True)) == ctr0 and ctr0["other_file"] >= 20 and ctr0["placed"] >= 20, ctr0
    files = gc.state_of(want["tag"]) != gc.NOMATCH
    assert set(want["fileid"][files]) == {0, 1}
    m.close()


def test_loud_errors():
    w = _workload()
    m, pairs, s1, s2, want, _ = _check(w, "whole")
    b1, b2, lo, hi = w["b1"], w["b2"], w["min_ins"], w["max_ins"]

    def status(**kw):
        with pytest.raises(rlib.RealHipError) as e:
            m.gap_rescue(b1, b2, pairs, s1, s2, kw.pop("min_ins", lo), kw.pop("max_ins", hi), **dict(_kw(w["prm"]), **kw))
        assert "gap rescue" in str(e.value) or "insert" in str(e.value), str(e.value)
        return e.value.status

    for bad in (dict(max_gap=0), dict(max_gap=17), dict(min_flank=0), dict(max_cost=65535), dict(cost_open=65536), dict(margin=1 << 16)):
        assert status(**bad) == rlib.REAL_HIP_E_INVALID, bad
    assert status(max_ins=rlib.REAL_HIP_MATE_SEARCH_MAX_INSERT + 1) == rlib.REAL_HIP_E_UNSUPPORTED
    assert status(min_ins=500, max_ins=400) == rlib.REAL_HIP_E_INVALID
    pp, gp = m._pair_params(lo, hi), m._gap_params(**_kw(w["prm"]))
    r1, r2 = m._mate_batch(b1), m._mate_batch(b2)
    out = new_gap_place(b1.n_reads)
    call = lambda *a: m._L.real_hip_gap_rescue(m._h, *a)                # noqa: E731
    args = [C.byref(pp), C.byref(gp), C.byref(r1), C.byref(r2), pairs.ctypes.data, s1.ctypes.data, s2.ctypes.data, 1, out.ctypes.data]
    for k in (0, 1, 2, 3, 4, 5, 6, 8):
        assert call(*[None if j == k else a for j, a in enumerate(args)]) == rlib.REAL_HIP_E_INVALID, k
    gp.struct_size -= 4
    assert call(*args) == rlib.REAL_HIP_E_INVALID
    gp.struct_size += 4
    gp.reserved[1] = 1
    assert call(*args) == rlib.REAL_HIP_E_INVALID
    gp.reserved[1] = 0
    short = m._mate_batch(b2.part(0, 5))
    assert call(*(args[:3] + [C.byref(short)] + args[4:])) == rlib.REAL_HIP_E_INVALID and "different numbers" in m._L.real_hip_last_error(m._h).decode()
    st = rlib.sized(rlib.RealHipGapStats)
    st.struct_size += 8
    assert m._L.real_hip_gap_stats_get(m._h, C.byref(st), 0) == rlib.REAL_HIP_E_INVALID
    assert out.tobytes() == new_gap_place(b1.n_reads).tobytes(), "nothing was launched"
    assert call(*args) == rlib.REAL_HIP_OK
    gc.assert_records_equal(out, want, "after the errors")
    m.close()
    # without a text
    bare = PairMatcher(RealOptions(seedl=gw.SEEDL, seedkmax=2, totalkmax=gw.TOTALKMAX, scores=False, filter_level=0).normalise())
    with pytest.raises(rlib.RealHipError) as e:
        bare.gap_rescue(b1, b2, pairs, s1, s2, lo, hi)
    assert e.value.status == rlib.REAL_HIP_E_STATE
    bare.close()
