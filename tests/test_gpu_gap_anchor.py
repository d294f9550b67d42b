"""Anchored gap placement on the device (real_hip_gap_anchor_hits, real_hip_match_gapped) against the checker of
gap_anchor_checker.py: every field of every record and every semantic counter, on info words that are the unchanged output of
real_hip_match_unique and hit lists that are the unchanged output of real_hip_match_all for the sub-read batch S(b, A)."""
import ctypes as C

import numpy as np
import pytest

import gap_anchor_checker as gac
import gap_anchor_workloads as gaw
import gap_checker as gc
import gapped_list_checker as glc
import indel_checker as ic
import pileup_checker as pk
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions, new_gap_place

pytestmark = pytest.mark.gpu


def _matcher(w, g=None, fileid=None, index=True):
    e = 1 if w["patl"] <= 33 else gaw.TOTALKMAX
    m = PairMatcher(RealOptions(seedl=w["seedl"], seedkmax=min(2, e), totalkmax=e, scores=False, filter_level=0).normalise())
    g = g or w["g"]
    m.set_text_symbols(w["fileid"] if fileid is None else fileid, g.sym, g.frag_start)
    if index:
        m.build_index_block()
    return m


def _kw(prm, ap):
    return dict(prm._asdict(), max_anchors=ap.max_anchors)


def _lists(m, w, a_len, info=None):
    """the final info words of the workload's reads (one file, one block) and the product's matchAll lists of S(b, A)"""
    b = w["b"]
    if info is None:
        info, _ = m.match_unique(b.bases, b.qual, b.offsets)
    sub = gac.SubBatch(b, a_len)
    hits, hoff = m.match_all(sub.bases, sub.qual, sub.offsets)
    return info, hits, hoff


def _counters(st):
    return {k: st[k] for k in gac.COUNTERS}


def _text(w, g=None, fileid=None):
    g = g or w["g"]
    return gc.Text(g.sym, g.frag_start, w["fileid"] if fileid is None else fileid)


def _check(w, ap, what, composite=True):
    """both entry points against the checker -> (matcher, info, hits, offsets, wanted records, wanted counters)"""
    m = _matcher(w)
    info, hits, hoff = _lists(m, w, ap.anchor_len)
    want, ctr = gac.check_anchor(_text(w), w["b"], info, hits, hoff, w["prm"], ap)
    print(what, ctr)
    keep = (info.copy(), hits.copy(), hoff.copy())
    got = m.gap_anchor_hits(w["b"], hits, hoff, ap.anchor_len, info=info, **_kw(w["prm"], ap))
    gac.assert_records_equal(got, want, what + ": gap_anchor_hits")
    st = m.gap_anchor_stats(reset=True)
    assert _counters(st) == ctr and st["launches"] == 2 and st["kernel_ms"] > 0, (st, ctr)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(keep, (info, hits, hoff))), "the records and lists are inputs"
    if composite:
        got = m.match_gapped(w["b"], ap.anchor_len, info=info, **_kw(w["prm"], ap))
        gac.assert_records_equal(got, want, what + ": match_gapped")
        st = m.gap_anchor_stats(reset=True)
        assert _counters(st) == ctr and st["launches"] == (3 if ctr["eligible"] > ctr["skipped"] else 1), (st, ctr)
    return m, info, hits, hoff, want, ctr


_W = {}


def _workload(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _W:
        _W[key] = gaw.workload(**kw)
    return _W[key]


def _anchor(w, max_anchors=32):
    return gac.AnchorParams(max(w["seedl"], gaw.default_anchor(w["patl"], w["prm"])), max_anchors)


# the shortest read searched (2 * min_flank + max_gap + 1), the word boundaries, the longest read, and one the stage skips
@pytest.mark.parametrize("patl", [25, 32, 33, 64, 65, 100, 320, 321])
def test_read_lengths_against_the_checker(patl):
    long = patl > 200
    w = _workload(seed=patl, patl=patl, n=80 if long else 150, size=200_000 if long else 150_000, per_class=3 if long else gaw.PER_CLASS)
    m, _, _, _, want, ctr = _check(w, _anchor(w), "patl %d" % patl)
    if patl == 321:
        assert ctr["skipped"] >= len(w["plants"]) and ctr["placed"] < ctr["eligible"] and ctr["gapped"] == 0
    else:
        assert ctr["gapped"] >= (5 if long else 10) and ctr["unique"] >= (5 if long else 10) and ctr["crowded"] >= 1, ctr
        assert long or {int(x) for x in gc.state_of(want["tag"])} == {0, 1, 2}
        assert {int(x) for x in gc.inverted_of(want["tag"][want["gap"] != 0])} == {0, 1}
    m.close()


# the seed's length, the longest anchor with full coverage, the whole read (nothing with a gap can anchor)
@pytest.mark.parametrize("a_len", [32, 46, 100])
def test_anchor_lengths_against_the_checker(a_len):
    w = _workload()
    m, _, _, _, want, ctr = _check(w, gac.AnchorParams(a_len, 32), "anchor_len %d" % a_len)
    if a_len == 100:
        assert ctr["gapped"] == 0 and ctr["unanchored"] >= 40, ctr
    else:
        assert ctr["gapped"] >= 30, ctr
    m.close()


@pytest.mark.parametrize("max_gap,margin,max_anchors", [(1, 0, 32), (16, 0, 32), (8, 3, 32), (8, 0, 1), (8, 0, 64)])
def test_gap_lengths_margin_and_anchor_budget_against_the_checker(max_gap, margin, max_anchors):
    w = _workload(seed=7, prm=gaw.default_params(max_gap=max_gap, margin=margin))
    m, _, _, _, want, ctr = _check(w, _anchor(w, max_anchors), "max_gap %d margin %d max_anchors %d" % (max_gap, margin, max_anchors))
    if max_anchors == 1:
        assert ctr["crowded"] >= 40 and ctr["placed"] >= 5, ctr                  # (one sub-read alone still anchors: classes P, S)
    else:
        assert ctr["gapped"] >= 10 and int(np.abs(want["gap"].astype(int)).max()) == max_gap
    m.close()


def test_hand_made_hit_lists():
    """lists the matcher would never return: every sub-read's hits backwards and once more, behind them a hit in a fragment
    that is none and one whose sub-read ends behind its fragment -- the same candidates, so the same records"""
    w = _workload()
    ap = _anchor(w, 64)
    m, info, hits, hoff, want, ctr = _check(w, ap, "the matcher's lists", composite=False)
    t = _text(w)
    parts, counts = [], []
    for s in range(hoff.shape[0] - 1):
        own = hits[int(hoff[s]):int(hoff[s + 1])]
        bad = np.zeros(2 if own.shape[0] and own.shape[0] <= 8 else 0, dtype=hits.dtype)
        if bad.shape[0]:
            bad[:] = own[0]
            bad[0]["frag"] = 60000
            f = int(own[0]["frag"])
            bad[1]["pos"] = t.frag_start[f + 1] - ap.anchor_len + 1
        lst = np.concatenate([own[::-1], own, bad]) if own.shape[0] <= 8 else own
        parts.append(lst)
        counts.append(lst.shape[0])
    hits2 = np.concatenate(parts)
    hoff2 = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    want2, ctr2 = gac.check_anchor(t, w["b"], info, hits2, hoff2, w["prm"], ap)
    got = m.gap_anchor_hits(w["b"], hits2, hoff2, ap.anchor_len, info=info, **_kw(w["prm"], ap))
    gac.assert_records_equal(got, want2, "hand-made lists")
    assert _counters(m.gap_anchor_stats(reset=True)) == ctr2
    assert ctr2["invalid_anchors"] >= 100 and ctr2["positions"] > ctr["positions"] and ctr2["anchors"] > ctr["anchors"], (ctr, ctr2)
    assert ctr2["crowded"] == ctr["crowded"] and want2.tobytes() == want.tobytes()      # (no list grew beyond max_anchors)
    m.close()


def test_null_info_batch_halves_and_where_the_arrays_live():
    import torch
    w = _workload()
    ap = _anchor(w)
    m, info, hits, hoff, want, ctr = _check(w, ap, "whole")
    b, kw = w["b"], _kw(w["prm"], ap)
    n_all = b.n_reads
    # info == NULL: every read is eligible, the ones the matcher places get their ungapped record
    want0, ctr0 = gac.check_anchor(_text(w), b, None, hits, hoff, w["prm"], ap)
    got = m.gap_anchor_hits(b, hits, hoff, ap.anchor_len, info=None, **kw)
    gac.assert_records_equal(got, want0, "info == NULL")
    assert _counters(m.gap_anchor_stats(reset=True)) == ctr0 and ctr0["eligible"] == n_all and ctr0["placed"] > ctr["placed"] + 50
    gac.assert_records_equal(m.match_gapped(b, ap.anchor_len, **kw), want0, "match_gapped, info == NULL")
    m.gap_anchor_stats(reset=True)
    # parts of the batch: the records of the whole, the counters add up
    half = n_all // 2 + 1
    for bounds in (((0, half), (half, n_all)), ((0, 0), (0, 1), (1, 66), (66, n_all))):
        parts = [m.match_gapped(b.part(lo, hi), ap.anchor_len, info=info[lo:hi], **kw) for lo, hi in bounds]
        gac.assert_records_equal(np.concatenate(parts), want, "parts %r" % (bounds,))
        assert _counters(m.gap_anchor_stats(reset=True)) == ctr
    parts = [m.gap_anchor_hits(b.part(lo, hi), hits[int(hoff[2 * lo]):int(hoff[2 * hi])], hoff[2 * lo:2 * hi + 1] - hoff[2 * lo], ap.anchor_len,
                               info=info[lo:hi], **kw) for lo, hi in ((0, half), (half, n_all))]
    gac.assert_records_equal(np.concatenate(parts), want, "two halves of the lists")
    assert _counters(m.gap_anchor_stats(reset=True)) == ctr
    # device reads, records and lists (on_device = 1), then device reads with host records (on_device = 2)
    dev = tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64)))
    dinfo, dhits, dhoff = (torch.from_numpy(x.view(np.uint8).copy()).cuda() for x in (info, hits, hoff))
    for call in (lambda o: m.gap_anchor_hits(dev, dhits, dhoff.view(torch.int64), ap.anchor_len, info=dinfo, out=o, fresh=True, **kw),
                 lambda o: m.match_gapped(dev, ap.anchor_len, info=dinfo, out=o, fresh=True, **kw)):
        out = torch.full((n_all * 16,), 0xAB, dtype=torch.uint8, device="cuda")
        call(out)
        gac.assert_records_equal(out.cpu().numpy().view(rlib.GAP_PLACE_DTYPE), want, "device arrays")
        assert _counters(m.gap_anchor_stats(reset=True)) == ctr
    gac.assert_records_equal(m.gap_anchor_hits(dev, hits, hoff, ap.anchor_len, info=info, **kw), want, "device reads, host records")
    gac.assert_records_equal(m.match_gapped(dev, ap.anchor_len, info=info, host_records=True, **kw), want, "device reads, host records, composite")
    m.close()


def test_packed_batches_with_a_read_starting_inside_a_byte():
    w = _workload()
    ap = _anchor(w)
    m, info, hits, hoff, want, ctr = _check(w, ap, "bytes")
    b = w["b"]
    packed = synth.pack_bases(np.concatenate([np.zeros(1, np.uint8), b.bases]))      # one base in front of everything
    flags, offs = synth.read_nflags(b.bases, b.offsets), (b.offsets + np.uint64(1)).astype(np.uint64)
    qual = np.concatenate([np.zeros(1, np.uint8), b.qual])
    rb = rlib.sized(rlib.RealHipBatch, on_device=0, n_reads=b.n_reads, bases=packed.ctypes.data, qual=qual.ctypes.data, offsets=offs.ctypes.data,
                    packed=1, nflags=flags.ctypes.data)
    gp, app = m._gap_params(**w["prm"]._asdict()), m._gap_anchor_params(ap.anchor_len, ap.max_anchors)
    for call in (lambda o: m._L.real_hip_gap_anchor_hits(m._h, C.byref(gp), C.byref(app), C.byref(rb), info.ctypes.data, hits.ctypes.data,
                                                         hoff.ctypes.data, 1, o.ctypes.data),
                 lambda o: m._L.real_hip_match_gapped(m._h, C.byref(gp), C.byref(app), C.byref(rb), info.ctypes.data, 1, o.ctypes.data)):
        out = new_gap_place(b.n_reads)
        out["pos"] = 77                                                      # (fresh: output only)
        m._check(call(out))
        gac.assert_records_equal(out, want, "packed, reads start inside a byte")
        assert _counters(m.gap_anchor_stats(reset=True)) == ctr
    m.close()


def _final_info(ws, files):
    """the final info words of the reads of ws[0]["b"] over the genome files [(genome, fileid)], one matcher each"""
    info = None
    for g, fid in files:
        m = _matcher(ws[0], g, fid)
        info, _ = m.match_unique(ws[0]["b"].bases, ws[0]["b"].qual, ws[0]["b"].offsets, info=info)
        m.close()
    return info


def test_two_genome_files_fold_in_both_orders():
    wa, wb = _workload(seed=1, n=60), _workload(seed=2, n=60, fileid=1)
    reads = [wa["b"].read(i) for i in range(wa["b"].n_reads)] + [wb["b"].read(i) for i in range(wb["b"].n_reads)]
    both = dict(wa, b=gaw.Batch(reads))
    ap = _anchor(both)
    kw = _kw(both["prm"], ap)
    files = [(wa["g"], 0), (wb["g"], 1)]
    info = _final_info([both], files)
    results = []
    for order in (files, files[::-1]):
        got = want = None
        for g, fid in order:
            m = _matcher(both, g, fid)
            _, hits, hoff = _lists(m, both, ap.anchor_len, info)
            want, ctr = gac.check_anchor(_text(both, g, fid), both["b"], info, hits, hoff, both["prm"], ap, out=want)
            got = m.match_gapped(both["b"], ap.anchor_len, info=info, out=got, **kw)
            gac.assert_records_equal(got, want, "file %d" % fid)
            assert _counters(m.gap_anchor_stats(reset=True)) == ctr and ctr["placed"] >= 40, ctr
            m.close()
        results.append(got)
    gac.assert_records_equal(results[0], results[1], "the two orders")
    placed = gc.state_of(results[0]["tag"]) != gc.NOMATCH
    assert set(results[0]["fileid"][placed]) == {0, 1}


def test_one_file_in_two_index_blocks_against_the_merge():
    w = _workload()
    ap = _anchor(w)
    kw = _kw(w["prm"], ap)
    b = w["b"]
    m = _matcher(w, index=False)
    blocks, first, more, per = [], 0, True, w["g"].n // 2 + 1
    while more:                                                             # blocks of half the text's windows each
        n_ent, more = m.build_index_block(first, per)
        blocks.append(first)
        first += n_ent
    assert len(blocks) >= 2
    info = None
    for first in blocks:
        m.build_index_block(first, per)
        info, _ = m.match_unique(b.bases, b.qual, b.offsets, info=info)
    got = want = None
    total = dict.fromkeys(gac.COUNTERS, 0)
    for first in blocks:
        m.build_index_block(first, per)
        _, hits, hoff = _lists(m, w, ap.anchor_len, info)
        want, ctr = gac.check_anchor(_text(w), b, info, hits, hoff, w["prm"], ap, out=want)
        got = m.match_gapped(b, ap.anchor_len, info=info, out=got, **kw)
        gac.assert_records_equal(got, want, "block at %d" % first)
        assert _counters(m.gap_anchor_stats(reset=True)) == ctr
        total = {k: total[k] + ctr[k] for k in total}
    assert total["placed"] >= 60 and total["gapped"] >= 40, total
    m.close()


def test_the_records_drive_the_gapped_lists_and_the_indel_calls():
    """the same batch given as both mates: tag bit 0 is 0, so the read is mate 1's"""
    w = _workload()
    ap = _anchor(w)
    b = w["b"]
    m, info, hits, hoff, want, ctr = _check(w, ap, "records", composite=False)
    gaps = m.match_gapped(b, ap.anchor_len, info=info, **_kw(w["prm"], ap))
    lists, off = m.mismatches_gapped(b, b, gaps)
    wl, woff, wctr = glc.gapped_lists(w["g"].sym, 0, b, b, want)
    assert off.tobytes() == woff.tobytes() and lists.tobytes() == wl.tobytes()
    st = m.gapped_list_stats(reset=True)
    assert {k: st[k] for k in glc.COUNTERS} == wctr and wctr["disagree"] == 0 and wctr["placed"] == ctr["unique"] and wctr["deleted"] > 20 and wctr["inserted"] > 20
    pu = pk.Pileup(w["g"].sym, 0, 20)
    pu.add(b, info)
    ind = ic.Indels(pu, w["g"].frag_start)
    ind.add(b, b, want)
    m.pileup_begin(20)
    m.pileup_add(b.bases, b.qual, info, b.offsets)
    m.pileup_finish()
    m.indel_begin()
    m.indel_add(b, b, gaps)
    m.indel_finish(20, 1, 1)
    ic.assert_lists_equal(m.indel_events(), ind.events(20, 1, 1), "events")
    ic.assert_lists_equal(m.indel_calls(), ind.calls(20, 1, 1), "calls")
    st = m.indel_stats()
    f = ind.finish_stats(20, 1, 1)
    assert {k: st[k] for k in f} == f and f["events"] >= 40 and f["invalid"] == 0, f
    m.indel_end()
    m.pileup_end()
    m.close()


def test_loud_errors():
    w = _workload()
    ap = _anchor(w)
    m, info, hits, hoff, want, _ = _check(w, ap, "whole", composite=False)
    b = w["b"]
    m.gap_anchor_stats(reset=True)

    def status(**kw):
        a_len = kw.pop("anchor_len", ap.anchor_len)
        codes = []
        for call in (lambda: m.gap_anchor_hits(b, hits, hoff, a_len, info=info, **dict(_kw(w["prm"], ap), **kw)),
                     lambda: m.match_gapped(b, a_len, info=info, **dict(_kw(w["prm"], ap), **kw))):
            with pytest.raises(rlib.RealHipError) as e:
                call()
            assert "anchored gap placement" in str(e.value), str(e.value)
            codes.append(e.value.status)
        assert codes[0] == codes[1]
        return codes[0]

    for bad in (dict(max_gap=0), dict(max_gap=17), dict(min_flank=0), dict(max_cost=65535), dict(cost_open=65536), dict(margin=1 << 16),
                dict(anchor_len=0), dict(anchor_len=321), dict(max_anchors=0), dict(max_anchors=65)):
        assert status(**bad) == rlib.REAL_HIP_E_INVALID, bad
    gp, app = m._gap_params(**w["prm"]._asdict()), m._gap_anchor_params(ap.anchor_len, ap.max_anchors)
    rb = m._mate_batch(b)
    out = new_gap_place(b.n_reads)
    call = lambda *a: m._L.real_hip_gap_anchor_hits(m._h, *a)                # noqa: E731
    comp = lambda *a: m._L.real_hip_match_gapped(m._h, *(a[:4] + a[6:]))      # noqa: E731
    args = [C.byref(gp), C.byref(app), C.byref(rb), info.ctypes.data, hits.ctypes.data, hoff.ctypes.data, 1, out.ctypes.data]
    for k in (0, 1, 2, 4, 5, 7):                                             # (info may be NULL)
        assert call(*[None if j == k else a for j, a in enumerate(args)]) == rlib.REAL_HIP_E_INVALID, k
    for k in (0, 1, 2, 7):
        assert comp(*[None if j == k else a for j, a in enumerate(args)]) == rlib.REAL_HIP_E_INVALID, k
    for s in (gp, app):
        s.struct_size -= 4
        assert call(*args) == comp(*args) == rlib.REAL_HIP_E_INVALID
        s.struct_size += 4
        s.reserved[1] = 1
        assert call(*args) == comp(*args) == rlib.REAL_HIP_E_INVALID
        s.reserved[1] = 0
    backwards = hoff.copy()
    backwards[5] = backwards[4] - 1 if backwards[4] else backwards[-1] + 1
    assert call(*(args[:5] + [backwards.ctypes.data] + args[6:])) == rlib.REAL_HIP_E_INVALID
    shifted = hoff + np.uint64(1)
    assert call(*(args[:5] + [shifted.ctypes.data] + args[6:])) == rlib.REAL_HIP_E_INVALID
    st = rlib.sized(rlib.RealHipGapAnchorStats)
    st.struct_size += 8
    assert m._L.real_hip_gap_anchor_stats_get(m._h, C.byref(st), 0) == rlib.REAL_HIP_E_INVALID
    assert out.tobytes() == new_gap_place(b.n_reads).tobytes() and m.gap_anchor_stats()["launches"] == 0, "nothing was launched"
    assert call(*args) == rlib.REAL_HIP_OK
    gac.assert_records_equal(out, want, "after the errors")
    m.close()
    # the composite needs an index block, the stage only the text; neither runs without a text
    noix = _matcher(w, index=False)
    gac.assert_records_equal(noix.gap_anchor_hits(b, hits, hoff, ap.anchor_len, info=info, **_kw(w["prm"], ap)), want, "the text alone")
    with pytest.raises(rlib.RealHipError) as e:
        noix.match_gapped(b, ap.anchor_len, info=info)
    assert e.value.status == rlib.REAL_HIP_E_STATE
    noix.close()
    bare = PairMatcher(RealOptions(seedl=32, seedkmax=2, totalkmax=3, scores=False, filter_level=0).normalise())
    for call in (lambda: bare.gap_anchor_hits(b, hits, hoff, ap.anchor_len, info=info), lambda: bare.match_gapped(b, ap.anchor_len, info=info)):
        with pytest.raises(rlib.RealHipError) as e:
            call()
        assert e.value.status == rlib.REAL_HIP_E_STATE
    bare.close()
