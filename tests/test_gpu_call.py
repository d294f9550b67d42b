"""The variant calls on the device (real_hip_call_*) against call_checker.py, which restates them in numpy over the ORACLE's
records.  The records handed to the library come from match_unique / match_pairs on the device and are first asserted to be
the oracle's / the pair checker's.  Evidence, calls and statistics are integers: everything is compared exactly."""
import ctypes as C
import types

import numpy as np
import pytest

import call_checker as ck
import call_workloads as cw
import dup_workloads as dw
import insert_workloads as iw
import pairs_checker as pc
import pileup_checker as pk
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions, UniqueMatcher

pytestmark = pytest.mark.gpu
COUNTS = ck.COUNTERS + ("calls", "het", "hom")


def _opts():
    return RealOptions(seedl=cw.SEEDL, seedkmax=cw.SEEDK, totalkmax=cw.TOTALK, scores=True, filter_level=cw.FILTER_LEVEL).normalise()


@pytest.fixture(scope="module")
def matched(ora):
    """(matcher with the workload's text and index, {batch name: its device-matched records}), the records asserted to be the
    oracle's"""
    import torch
    torch.zeros(1, device="cuda")      # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    w = cw.workload()
    m = UniqueMatcher(_opts())
    m.set_text_symbols(0, w.g.sym, w.g.frag_start)
    m.build_index_block()
    rec = {}
    for which in cw.BATCHES:
        b = getattr(w, which)
        info, _ = m.match_unique(b.bases, b.qual, offsets=b.offsets)
        assert np.array_equal(info, cw.oracle_records(ora, which)), which
        rec[which] = info
    yield m, rec
    m.close()


def _add(m, what, b, info, packed=False, on_device=0):
    """one pileup_add / call_add (what) of the batch in the form asked for"""
    import torch
    bases, nflags = (synth.pack_bases(b.bases), synth.read_nflags(b.bases, b.offsets)) if packed else (b.bases, None)
    qual, off = b.qual, b.offsets
    if on_device:
        bases, off = torch.from_numpy(bases).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        qual = None if qual is None else torch.from_numpy(qual).cuda()
        nflags = None if nflags is None else torch.from_numpy(nflags).cuda()
        if on_device == 1:
            info = torch.from_numpy(info.view(np.int64)).cuda()
    getattr(m, what)(bases, qual, info, offsets=off, packed=packed, nflags=nflags)


def _pile(m, min_qual, adds, packed=False, on_device=0):
    """a finished pileup of the (batch, records) in adds"""
    m.pileup_begin(min_qual)
    for b, info in adds:
        _add(m, "pileup_add", b, info, packed, on_device)
    return m.pileup_finish()


def _equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    for k in want.dtype.names:
        assert np.array_equal(got[k], want[k]), (what, k, np.nonzero((got[k] != want[k]).reshape(got.shape[0], -1).any(axis=1))[0][:10])


def _compare(m, cl, adds, what, thresholds=(20, 4), same_records=True):
    """finish, then evidence, calls and every count against the checker's; the launches: begin, the adds, count and scan, emit.
    same_records: the calls were given what the pileup was given, so that the two kernels' counts of the other bases agree"""
    n_calls = m.call_finish(*thresholds)
    want = cl.calls(*thresholds)
    ev, calls, sites = m.call_evidence(), m.call_variants(), m.pileup_sites()
    _equal(sites, cl.site_list, (what, "sites"))
    _equal(ev, cl.evidence(), (what, "evidence"))
    other = np.arange(4)[None, :] != sites["ref"][:, None]
    assert not same_records or np.array_equal(ev["cnt"][other], sites["alt"][other]), (what, "cnt[s][b] == site.alt[b] for b != ref")
    assert n_calls == want.shape[0], (what, n_calls, want.shape[0])
    _equal(calls, want, (what, "calls"))
    st = m.call_stats(reset=True)
    wst = cl.finish_stats(*thresholds)
    assert {k: st[k] for k in COUNTS} == wst, (what, st, wst)
    if adds is not None:
        n_sites = cl.site_list.shape[0]
        assert st["launches"] == 1 + adds + (2 + (1 if n_calls else 0) if n_sites else 0) and st["kernel_ms"] > 0, (what, st)
    return calls


@pytest.mark.parametrize("min_qual", [0, 20])
@pytest.mark.parametrize("on_device", [0, 1, 2])
@pytest.mark.parametrize("packed", [False, True])
def test_calls_of_the_workload(ora, matched, packed, on_device, min_qual):
    """the 40x batch, the ragged batch with its hot spot and the long reads: three adds"""
    m, rec = matched
    w = cw.workload()
    pu, cl = cw.expected(ora, cw.BATCHES, min_qual)
    adds = [(getattr(w, k), rec[k]) for k in cw.BATCHES]
    assert _pile(m, min_qual, adds, packed, on_device) == cl.site_list.shape[0] > 10_000
    m.call_stats(reset=True)
    m.call_begin()
    for b, info in adds:
        _add(m, "call_add", b, info, packed, on_device)
    calls = _compare(m, cl, 3, (packed, on_device, min_qual))
    m.call_end()
    m.pileup_end()
    at = set(calls["pos"].tolist())
    assert set(w.forced) <= at and calls.shape[0] >= 150 and (calls["a1"] != calls["a2"]).sum() >= 90 and (cl.stats["low_qual"] > 10_000) == (min_qual > 0)


def test_one_add_is_three_adds_and_finish_again_with_other_thresholds(ora, matched):
    m, rec = matched
    w = cw.workload()
    pu, cl = cw.expected(ora, cw.BATCHES, 20)
    adds = [(getattr(w, k), rec[k]) for k in cw.BATCHES]
    whole = synth.concat_batches([b for b, _ in adds])
    assert whole.offsets[-1] == sum(int(b.offsets[-1]) for b, _ in adds)
    info = np.concatenate([r for _, r in adds])
    _pile(m, 20, adds)
    m.call_stats(reset=True)
    m.call_begin()
    _add(m, "call_add", whole, info, packed=True, on_device=2)
    _compare(m, cl, 1, "one add")
    # finish again: other thresholds, no new adds -- it only re-reads the evidence (the counters of the adds were reset above)
    zero = {k: 0 for k in ck.COUNTERS}
    for th in ((0, 0), (20, 4), (300, 4), (20, 60), (1 << 31, 0)):
        n_calls = m.call_finish(*th)
        want = cl.calls(*th)
        assert n_calls == want.shape[0] and (th != (0, 0) or n_calls > 200) and (th != (1 << 31, 0) or n_calls == 0), (th, n_calls)
        _equal(m.call_variants(), want, th)
        _equal(m.call_evidence(), cl.evidence(), th)
        st = m.call_stats(reset=True)
        fs = cl.finish_stats(*th)
        assert {k: st[k] for k in COUNTS} == dict(zero, calls=fs["calls"], het=fs["het"], hom=fs["hom"]) and st["launches"] == 2 + (1 if n_calls else 0), (th, st)
    with pytest.raises(rlib.RealHipError, match="add after finish"):
        _add(m, "call_add", w.long, rec["long"])
    m.call_end()
    m.pileup_end()


def test_begin_again_starts_from_zero_and_long_reads_alone(ora, matched):
    """a second call_begin on the same pileup: the evidence of what came before is gone"""
    m, rec = matched
    w = cw.workload()
    pu, _ = cw.expected(ora, cw.BATCHES, 20)
    _pile(m, 20, [(getattr(w, k), rec[k]) for k in cw.BATCHES])
    m.call_stats(reset=True)
    m.call_begin()
    _add(m, "call_add", w.cov, rec["cov"])
    m.call_finish()
    first = m.call_stats(reset=True)
    assert first["calls"] > 100 and first["site_bases"] > 100_000
    for packed in (False, True):
        cl = ck.Calls(pu)                                               # the long reads alone over the sites of everything
        cl.add(w.long, cw.oracle_records(ora, "long"))
        assert cl.stats["site_bases"] > 3000
        m.call_begin()
        _add(m, "call_add", w.long, rec["long"], packed=packed)
        _compare(m, cl, 1, ("begin again, long reads", packed), thresholds=(0, 1), same_records=False)
    m.call_end()
    m.pileup_end()


def test_records_of_another_file_are_skipped_and_counted(ora, matched):
    m, rec = matched
    w = cw.workload()
    other = cw.oracle_records(ora, "ragged", fileid=1)
    st = ora.unpack_record(other)
    assert (st[3][(st[0] == 1) | (st[0] == 2)] == 1).all()
    mixed = np.where(np.arange(other.shape[0]) % 3 == 0, other, rec["ragged"])
    pu = pk.Pileup(w.g.sym, 0, 0)
    pu.add(w.ragged, mixed)
    cl = ck.Calls(pu)
    cl.add(w.ragged, mixed)
    assert cl.stats["other_file"] > 500 and cl.stats["placed"] > 1000
    _pile(m, 0, [(w.ragged, mixed)])
    m.call_stats(reset=True)
    m.call_begin()
    _add(m, "call_add", w.ragged, mixed)
    _compare(m, cl, 1, "two file ids")
    m.call_end()
    m.pileup_end()


@pytest.mark.parametrize("packed,on_device", [(False, 0), (True, 1)])
def test_batch_without_qualities_counts_as_quality_30(ora, matched, packed, on_device):
    m, rec = matched
    w = cw.workload()
    b = types.SimpleNamespace(bases=w.ragged.bases, qual=None, offsets=w.ragged.offsets)
    for min_qual in (30, 31):
        pu = pk.Pileup(w.g.sym, 0, min_qual)
        pu.add(b, cw.oracle_records(ora, "ragged"))
        cl = ck.Calls(pu)
        cl.add(b, cw.oracle_records(ora, "ragged"))
        if min_qual == 30:
            assert cl.stats["site_bases"] > 10_000 and cl.stats["low_qual"] == 0 and (cl.qsum == 30 * cl.cnt).all() and cl.calls().shape[0] > 5
        else:
            assert cl.site_list.shape[0] == 0 and cl.stats["site_bases"] == 0 and cl.stats["placed"] > 1500      # zero sites
        assert _pile(m, min_qual, [(b, rec["ragged"])], packed, on_device) == cl.site_list.shape[0]
        m.call_stats(reset=True)
        m.call_begin()
        _add(m, "call_add", b, rec["ragged"], packed, on_device)
        _compare(m, cl, 1, ("no qualities", packed, on_device, min_qual))
    m.call_end()
    m.pileup_end()


def test_zero_sites_is_valid(matched):
    """a finished pileup nothing was added to: the adds still count their placements, finish launches nothing"""
    m, rec = matched
    w = cw.workload()
    assert _pile(m, 0, []) == 0
    m.call_stats(reset=True)
    m.call_begin()
    _add(m, "call_add", w.long, rec["long"])
    assert m.call_finish() == 0 and m.call_evidence().shape[0] == 0 and m.call_variants().shape[0] == 0
    st = m.call_stats(reset=True)
    assert st["placed"] == 42 and st["site_bases"] == 0 and st["low_qual"] == 0 and st["calls"] == 0 and st["launches"] == 2, st
    m.call_end()
    m.pileup_end()


def test_both_capacity_protocols(ora, matched):
    import torch
    m, rec = matched
    w = cw.workload()
    pu = pk.Pileup(w.g.sym, 0, 20)
    pu.add(w.ragged, cw.oracle_records(ora, "ragged"))
    cl = ck.Calls(pu)
    cl.add(w.ragged, cw.oracle_records(ora, "ragged"))
    _pile(m, 20, [(w.ragged, rec["ragged"])])
    m.call_begin()
    _add(m, "call_add", w.ragged, rec["ragged"])
    want = {"evidence": cl.evidence(), "variants": cl.calls(0, 1)}
    assert m.call_finish(0, 1) == want["variants"].shape[0] > 20 and want["evidence"].shape[0] > 500
    nout = C.c_uint64(0)
    for name, call, dtype, key in (("evidence", m._L.real_hip_call_evidence, rlib.CALL_EVIDENCE_DTYPE, "cnt"), ("variants", m._L.real_hip_call_variants, rlib.CALL_DTYPE, "pos")):
        total = want[name].shape[0]
        out = np.full(total + 1, 7, dtype=dtype)
        for cap in (0, 1, total - 1):
            assert call(m._h, out.ctypes.data, cap, C.byref(nout), 0) == rlib.REAL_HIP_E_OVERFLOW and nout.value == total
            assert (out[key] == 7).all(), "nothing is written on overflow"
        nout.value = 0
        assert call(m._h, out.ctypes.data, total, C.byref(nout), 0) == rlib.REAL_HIP_OK and nout.value == total
        _equal(out[:-1], want[name], name)
        assert (out[key][-1] == 7).all()
        dev = torch.zeros(total * 32, dtype=torch.uint8, device="cuda")
        assert call(m._h, dev.data_ptr(), total, C.byref(nout), 1) == rlib.REAL_HIP_OK
        _equal(dev.cpu().numpy().view(dtype), want[name], (name, "on the device"))
    _equal(m.call_evidence(cap=1), want["evidence"], "the mirror grows its buffer once")
    _equal(m.call_variants(cap=1), want["variants"], "the mirror grows its buffer once")
    m.call_end()
    m.pileup_end()


def test_call_errors_are_loud_and_launch_nothing(ora, matched):
    m, rec = matched
    w = cw.workload()
    a = (w.long, rec["long"])

    def refused(word, call):
        before = m.call_stats()
        with pytest.raises(rlib.RealHipError, match=word) as e:
            call()
        assert e.value.status == rlib.REAL_HIP_E_INVALID
        after = m.call_stats()
        assert after["launches"] == before["launches"] and after["reads"] == before["reads"], word

    m.pileup_end()
    m.call_stats(reset=True)
    refused("needs a finished pileup", m.call_begin)
    refused("add without begin", lambda: _add(m, "call_add", *a))
    refused("finish without begin", m.call_finish)
    refused("before finish", m.call_evidence)
    refused("before finish", m.call_variants)
    m.pileup_begin(0)
    _add(m, "pileup_add", *a)
    refused("needs a finished pileup", m.call_begin)                   # begun, not finished
    m.pileup_finish()
    m.call_begin()
    refused("before finish", m.call_evidence)
    refused("before finish", m.call_variants)
    _add(m, "call_add", *a)
    # more than 2^32 reads in one call: refused on the count alone (no array is looked at)
    big = rlib.RealHipBatch()
    big.struct_size, big.n_reads, big.patl = C.sizeof(rlib.RealHipBatch), (1 << 32) + 1, 50
    dummy = np.zeros(8, dtype=np.uint64)
    big.bases = dummy.ctypes.data
    refused("more than 2\\^32 reads", lambda: m._check(m._L.real_hip_call_add(m._h, C.byref(big), dummy.ctypes.data)))
    refused("more than 2\\^32 reads", lambda: m._check(m._L.real_hip_call_add_pairs(m._h, C.byref(big), C.byref(big), dummy.ctypes.data)))
    bad = rlib.RealHipCallParams()
    bad.struct_size = 8
    refused("struct_size", lambda: m._check(m._L.real_hip_call_finish(m._h, C.byref(bad), None)))
    m.call_finish()
    refused("add after finish", lambda: _add(m, "call_add", *a))
    pu = pk.Pileup(w.g.sym, 0, 0)
    pu.add(*[a[0], cw.oracle_records(ora, "long")])
    cl = ck.Calls(pu)
    cl.add(a[0], cw.oracle_records(ora, "long"))
    _equal(m.call_evidence(), cl.evidence(), "the refused calls changed nothing")
    # the pileup's end and a new pileup begin end the calls as well
    m.pileup_end()
    refused("before finish", m.call_variants)
    refused("add without begin", lambda: _add(m, "call_add", *a))
    _pile(m, 0, [a])
    m.call_begin()
    m.pileup_begin(0)
    refused("add without begin", lambda: _add(m, "call_add", *a))
    refused("finish without begin", m.call_finish)
    m.pileup_end()
    # the text replaced by one of another length, then by one of another file id: begin, add and finish are refused
    m2 = UniqueMatcher(_opts())
    for fileid, sym, fs in ((0, w.g.sym[:-5], np.array([0, w.g.n - 5], dtype=np.uint64)), (3, w.g.sym, w.g.frag_start)):
        for begun in (False, True):
            m2.set_text_symbols(0, w.g.sym, w.g.frag_start)
            _pile(m2, 0, [a])
            if begun:
                m2.call_begin()
            m2.call_stats(reset=True)
            m2.set_text_symbols(fileid, sym, fs)
            for call in ((lambda: _add(m2, "call_add", *a), m2.call_finish) if begun else (m2.call_begin,)):
                with pytest.raises(rlib.RealHipError, match="text was replaced") as e:
                    call()
                assert e.value.status == rlib.REAL_HIP_E_INVALID and m2.call_stats()["launches"] == 0
    m2.close()


# ---- hand-made records: what no matcher writes -- placements that end at n, one base behind it, and of another file ----------
def _info(state, pos, fileid=0):
    return (state << 61) | (fileid << 35) | pos


def _hand_batch(g, places, seed):
    """reads that fit the text at (position, length, reverse strand) with a substitution every 13th text position and qualities
    0..40; a placement that does not fit gets random bases"""
    rng = np.random.default_rng(seed)
    ref = np.where(g.sym > 3, 0, g.sym).astype(np.uint8)
    reads, quals = [], []
    for p, L, inv in places:
        if p + L > g.n:
            o = rng.integers(0, 4, size=L).astype(np.uint8)
        else:
            x = np.arange(p, p + L)
            o = ref[x].copy()
            o[x % 13 == 0] = (o[x % 13 == 0] + 1 + (p % 3)) & 3
        reads.append(synth.revcomp(o) if inv else o)
        quals.append(rng.integers(0, 41, size=L).astype(np.uint8))
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    return types.SimpleNamespace(bases=np.concatenate(reads), qual=np.concatenate(quals), offsets=off)


@pytest.mark.parametrize("min_qual", [0, 20])
@pytest.mark.parametrize("packed,on_device", [(False, 0), (True, 0), (False, 1), (True, 2)])
def test_hand_made_records_at_the_end_of_the_text_and_behind_it(matched, packed, on_device, min_qual):
    m, _ = matched
    g = cw.workload().g
    n = g.n
    fit = [(p, L, inv) for p, L in ((n - 100, 100), (n - 33, 33), (n - 64, 64), (n - 320, 320), (n - 1, 1), (0, 65), (0, 1), (n - 700, 700), (n - 101, 100))
           for inv in (False, True)]
    beyond = [(n - 32, 33, False), (n, 40, True), (n - 99, 100, True), ((1 << 33) + 5, 50, False), (n - 699, 700, False)]      # by one base; at n; 35 bits of position
    foreign = [(n - 100, 100, False), (5, 80, True)]
    places = fit[:6] + beyond[:2] + foreign[:1] + fit[6:] + beyond[2:] + foreign[1:]
    b = _hand_batch(g, places, 11)
    info = np.array([_info(2 if inv else 1, p, 1 if k in (8, len(places) - 1) else 0) for k, (p, _, inv) in enumerate(places)], dtype=np.uint64)
    pu = pk.Pileup(g.sym, 0, min_qual)
    pu.add(b, info)
    cl = ck.Calls(pu)
    cl.add(b, info)
    assert cl.stats["invalid"] == len(beyond) and cl.stats["placed"] == len(fit) and cl.stats["other_file"] == 2 and pu.depth[n - 1] >= 10
    assert (cl.site_list["pos"] == n - 1 - (n - 1) % 13).any() and (min_qual or cl.site_list["pos"][0] == 0) and (cl.stats["low_qual"] > 0) == (min_qual > 0)
    _pile(m, min_qual, [(b, info)], packed, on_device)
    m.call_stats(reset=True)
    m.call_begin()
    _add(m, "call_add", b, info, packed, on_device)
    calls = _compare(m, cl, 1, ("hand-made", packed, on_device, min_qual), thresholds=(0, 1))
    assert calls.shape[0] > 20
    m.call_end()
    m.pileup_end()


@pytest.mark.parametrize("on_device", [0, 1])
def test_hand_made_pairs_both_mates_over_one_site(matched, on_device):
    """mates of different lengths that overlap over a site (both count), one with mate 2 behind the text (mate 1 still counts),
    one of another file, one NonUnique"""
    import torch
    m, _ = matched
    g = cw.workload().g
    n = g.n
    p1 = [(1300, 100, False), (2600, 64, True), (n - 300, 100, False), (n - 50, 51, True), (3900, 33, True), (100, 50, False), (5200, 90, False)]
    p2 = [(1340, 80, True), (2590, 120, False), (n - 99, 100, True), (n - 10, 11, False), (3900, 700, False), (300, 60, True), (5230, 70, True)]
    b1, b2 = _hand_batch(g, p1, 6), _hand_batch(g, p2, 7)
    pairs = np.zeros(len(p1), dtype=rlib.PAIR_DTYPE)
    pairs["pos1"], pairs["pos2"] = [x[0] for x in p1], [x[0] for x in p2]
    pairs["inverted1"] = [int(x[2]) for x in p1]
    pairs["state"] = [pc.UNIQUE] * 5 + [pc.NONUNIQUE, pc.UNIQUE]
    pairs["fileid"][6] = 1
    for min_qual in (0, 20):
        pu = pk.Pileup(g.sym, 0, min_qual)
        pu.add_pairs(b1, b2, pairs)
        cl = ck.Calls(pu)
        cl.add_pairs(b1, b2, pairs)
        assert cl.stats == dict(cl.stats, reads=14, placed=7, invalid=3, other_file=2)
        both = cl.site_list["pos"] == 1352                                  # 13 * 104: under both mates of pair 0
        assert pu.depth[1352] == 2 and (min_qual or (both.sum() == 1 and cl.cnt[both].sum() == 2 and (cl.cnt[both] == 1).sum() == 2))
        _equal(_pile_pairs(m, min_qual, b1, b2, pairs, on_device), cl.site_list, "sites")
        m.call_stats(reset=True)
        m.call_begin()
        _add_pairs(m, "call_add_pairs", b1, b2, pairs, on_device)
        _compare(m, cl, 2, ("hand-made pairs", on_device, min_qual), thresholds=(0, 1))
    m.call_end()
    m.pileup_end()


def _add_pairs(m, what, b1, b2, pairs, on_device):
    import torch
    if on_device:
        dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)]
        getattr(m, what)(dev[0], dev[1], torch.from_numpy(pairs.view(np.uint8).copy()).cuda())
    else:
        getattr(m, what)((b1.bases, b1.qual, b1.offsets), (b2.bases, b2.qual, b2.offsets), pairs)


def _pile_pairs(m, min_qual, b1, b2, pairs, on_device):
    m.pileup_begin(min_qual)
    _add_pairs(m, "pileup_add_pairs", b1, b2, pairs, on_device)
    m.pileup_finish()
    return m.pileup_sites()


@pytest.mark.parametrize("on_device", [0, 1])
def test_calls_of_pairs(ora, on_device):
    """PairMatcher.match_pairs on the duplicate workload's pairs (ragged mates, copies of fragments, qualities 0..40), its
    records asserted to be the pair checker's, then the evidence of both mates of every Unique record"""
    g, b1, b2 = dw.pair_workload()
    rec = dw.pair_expected(ora)[0]
    l1, l2 = (b.offsets[1:] - b.offsets[:-1] for b in (b1, b2))
    m = PairMatcher(RealOptions(seedl=iw.SEEDL, seedkmax=2, totalkmax=iw.TOTALK, scores=True, filter_level=iw.FILTER_LEVEL).normalise())
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    pairs = m.match_pairs(b1, b2, iw.WINDOW[0], iw.WINDOW[1])
    pc.assert_records_equal(pairs, rec, "match_pairs")
    uniq = rec["state"] == pc.UNIQUE
    assert uniq.sum() > 1000 and (l1[uniq] != l2[uniq]).sum() > 500 and (rec["inverted1"][uniq] == 1).sum() > 300
    for min_qual in (0, 10):
        pu = pk.Pileup(g.sym, 0, min_qual)
        pu.add_pairs(b1, b2, rec)
        cl = ck.Calls(pu)
        cl.add_pairs(b1, b2, rec)
        assert cl.stats["placed"] == 2 * int(uniq.sum()) and cl.stats["site_bases"] > (200 if min_qual else 1000) and (cl.stats["low_qual"] > 100) == (min_qual > 0)
        assert cl.calls(0, 1).shape[0] > 20
        _equal(_pile_pairs(m, min_qual, b1, b2, pairs, on_device), cl.site_list, "sites")
        m.call_stats(reset=True)
        m.call_begin()
        _add_pairs(m, "call_add_pairs", b1, b2, pairs, on_device)
        _compare(m, cl, 2, ("pairs", on_device, min_qual), thresholds=(0, 1))
    m.close()
