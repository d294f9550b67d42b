"""The pileup on the device (real_hip_pileup_*) against pileup_checker.py, which restates it in numpy over the ORACLE's
records.  The records handed to the library come from match_unique / match_pairs on the device and are first asserted to be
the oracle's / the pair checker's.  Depth, sites and statistics are integers: everything is compared exactly."""
import ctypes as C
import types

import numpy as np
import pytest

import insert_workloads as iw
import pairs_checker as pc
import pileup_checker as pk
import pileup_workloads as pw
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions, UniqueMatcher

pytestmark = pytest.mark.gpu
COUNTS = pk.COUNTERS + ("covered", "sites", "max_depth")


def _opts(scores):
    return RealOptions(seedl=pw.SEEDL, seedkmax=pw.SEEDK, totalkmax=pw.TOTALK, scores=bool(scores), filter_level=pw.FILTER_LEVEL).normalise()


@pytest.fixture(scope="module")
def matchers(ora):
    """scores -> (matcher with the workload's text and index, {batch name: its device-matched records}), the records asserted
    to be the oracle's"""
    import torch
    torch.zeros(1, device="cuda")      # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    w = pw.workload()
    out = {}
    for scores in (1, 0):
        m = UniqueMatcher(_opts(scores))
        m.set_text_symbols(0, w.g.sym, w.g.frag_start)
        m.build_index_block()
        rec = {}
        for which in ("main", "long"):
            b = getattr(w, which)
            info, score = m.match_unique(b.bases, b.qual, offsets=b.offsets)
            oinfo, oscore = pw.oracle_records(ora, which, scores)
            assert np.array_equal(info, oinfo), (which, scores)
            assert not scores or np.array_equal(score.view(np.uint32), oscore.view(np.uint32))
            rec[which] = info
        out[scores] = (m, rec)
    yield out
    for m, _ in out.values():
        m.close()


def _slice(b, lo, hi):
    a, e = int(b.offsets[lo]), int(b.offsets[hi])
    return types.SimpleNamespace(bases=b.bases[a:e], qual=b.qual[a:e], offsets=(b.offsets[lo:hi + 1] - b.offsets[lo]).astype(np.uint64))


def _add(m, b, info, packed=False, on_device=0):
    """one pileup_add of the batch in the form asked for"""
    import torch
    bases, nflags = (synth.pack_bases(b.bases), synth.read_nflags(b.bases, b.offsets)) if packed else (b.bases, None)
    qual, off = b.qual, b.offsets
    if on_device:
        bases, off = torch.from_numpy(bases).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        qual = None if qual is None else torch.from_numpy(qual).cuda()
        nflags = None if nflags is None else torch.from_numpy(nflags).cuda()
        if on_device == 1:
            info = torch.from_numpy(info.view(np.int64)).cuda()
    m.pileup_add(bases, qual, info, offsets=off, packed=packed, nflags=nflags)


def _compare(m, want, adds, what, one_begin=True):
    """depth, sites and every count of the finished pileup against the checker's; one_begin: the counters cover what was added
    since the last begin and nothing else, so that the depths sum to `bases`"""
    n = want.n
    n_sites = m.pileup_finish()
    depth = m.pileup_depth(0, n)
    sites = m.pileup_sites()
    st = m.pileup_stats(reset=True)
    assert depth.dtype == np.uint32 and np.array_equal(depth, want.depth), (what, np.nonzero(depth != want.depth)[0][:10])
    ws = want.sites()
    assert n_sites == ws.shape[0] == sites.shape[0], (what, n_sites, ws.shape[0])
    for k in ("pos", "depth", "alt", "ref", "reserved"):
        assert np.array_equal(sites[k], ws[k]), (what, k)
    wst = want.finish_stats()
    assert {k: st[k] for k in COUNTS} == wst, (what, st, wst)
    assert not one_begin or int(depth.astype(np.int64).sum()) == st["bases"]
    assert st["launches"] == adds + 3 + (1 if n_sites else 0) and st["kernel_ms"] > 0, (what, st)


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("min_qual", [0, 20])
@pytest.mark.parametrize("on_device", [0, 1, 2])
@pytest.mark.parametrize("packed", [False, True])
def test_pileup_of_the_workload(ora, matchers, packed, on_device, min_qual, scores):
    m, rec = matchers[scores]
    want = pw.expected(ora, "main", scores, min_qual)
    m.pileup_stats(reset=True)
    m.pileup_begin(min_qual)
    _add(m, pw.workload().main, rec["main"], packed, on_device)
    _compare(m, want, 1, (packed, on_device, min_qual, scores))
    m.pileup_end()
    assert want.finish_stats()["max_depth"] >= 300 and want.stats["placed"] > 1500 and (not min_qual or want.stats["low_qual"] > 100)


@pytest.mark.parametrize("packed", [False, True])
def test_pileup_of_long_reads(ora, matchers, packed):
    m, rec = matchers[1]
    for min_qual in (0, 20):
        want = pw.expected(ora, "long", 1, min_qual)
        assert want.stats["placed"] >= 30 and want.stats["mismatches"] > 20
        m.pileup_stats(reset=True)
        m.pileup_begin(min_qual)
        _add(m, pw.workload().long, rec["long"], packed, 0)
        _compare(m, want, 1, ("long", packed, min_qual))
    m.pileup_end()


def test_two_adds_are_one_add_and_begin_starts_again(ora, matchers):
    m, rec = matchers[1]
    w = pw.workload()
    cut = 1111
    a, b = _slice(w.main, 0, cut), _slice(w.main, cut, w.main.n_reads)
    whole = pk.Pileup(w.g.sym, 0, 20)
    whole.add(w.main, pw.oracle_records(ora, "main", 1)[0])
    whole.add(w.long, pw.oracle_records(ora, "long", 1)[0])
    m.pileup_stats(reset=True)
    m.pileup_begin(20)
    _add(m, a, rec["main"][:cut])
    _add(m, w.long, rec["long"], packed=True, on_device=2)
    _add(m, b, rec["main"][cut:], on_device=1)
    _compare(m, whole, 3, "three adds")
    # begin again: from zero, with another min_qual, whatever the accumulators held
    m.pileup_begin(0)
    _add(m, a, rec["main"][:cut])
    m.pileup_begin(0)
    _add(m, b, rec["main"][cut:])
    second = pk.Pileup(w.g.sym, 0, 0)
    second.add(b, pw.oracle_records(ora, "main", 1)[0][cut:])
    first = pk.Pileup(w.g.sym, 0, 0)
    first.add(a, pw.oracle_records(ora, "main", 1)[0][:cut])
    for k in pk.COUNTERS:                           # (the counters run on since the last reset: the first half was looked at and
        second.stats[k] += first.stats[k]           # counted; depth, sites, covered and max_depth are the second half's alone)
    _compare(m, second, 2, "begin again", one_begin=False)
    m.pileup_end()


def test_records_of_another_file_are_skipped_and_counted(ora, matchers):
    m, rec = matchers[1]
    w = pw.workload()
    other = pw.oracle_records(ora, "main", 1, fileid=1)[0]
    st = ora.unpack_record(other)
    assert (st[3][(st[0] == 1) | (st[0] == 2)] == 1).all()
    mixed = np.where(np.arange(other.shape[0]) % 3 == 0, other, rec["main"])
    want = pk.Pileup(w.g.sym, 0, 0)
    want.add(w.main, mixed)
    assert want.stats["other_file"] > 500 and want.stats["placed"] > 1000
    m.pileup_stats(reset=True)
    m.pileup_begin(0)
    _add(m, w.main, mixed)
    _compare(m, want, 1, "two file ids")
    m.pileup_end()


def test_sites_capacity_and_depth_windows(ora, matchers):
    m, rec = matchers[1]
    w = pw.workload()
    want = pw.expected(ora, "main", 1, 0)
    n, ws = want.n, want.sites()
    m.pileup_begin(0)
    _add(m, w.main, rec["main"])
    assert m.pileup_finish() == ws.shape[0] > 100
    out = np.full(ws.shape[0] + 1, 7, dtype=rlib.PILEUP_SITE_DTYPE)
    nout = C.c_uint64(0)
    call = m._L.real_hip_pileup_sites
    for cap in (0, 1, ws.shape[0] - 1):
        assert call(m._h, out.ctypes.data, cap, C.byref(nout), 0) == rlib.REAL_HIP_E_OVERFLOW and nout.value == ws.shape[0]
        assert (out["pos"] == 7).all(), "nothing is written on overflow"
    assert call(m._h, out.ctypes.data, ws.shape[0], C.byref(nout), 0) == rlib.REAL_HIP_OK and nout.value == ws.shape[0]
    assert np.array_equal(out["pos"][:-1], ws["pos"]) and out["pos"][-1] == 7
    assert np.array_equal(m.pileup_sites(cap=1)["alt"], ws["alt"])          # the mirror grows its buffer once
    import torch
    dev = torch.zeros(ws.shape[0] * 32, dtype=torch.uint8, device="cuda")
    assert call(m._h, dev.data_ptr(), ws.shape[0], C.byref(nout), 1) == rlib.REAL_HIP_OK
    assert np.array_equal(dev.cpu().numpy().view(rlib.PILEUP_SITE_DTYPE)["depth"], ws["depth"])
    # windows at both ends of the text, an empty one behind its end, and on the device
    assert np.array_equal(m.pileup_depth(0, 100), want.depth[:100]) and np.array_equal(m.pileup_depth(n - 100, 100), want.depth[-100:])
    assert want.depth[0] > 0 and want.depth[-1] > 0
    assert np.array_equal(m.pileup_depth(n - 1, 1), want.depth[-1:]) and m.pileup_depth(n, 0).shape[0] == 0
    dd = torch.zeros(300, dtype=torch.int32, device="cuda")
    m.pileup_depth(pw.HOT_AT - 100, 300, out=dd)
    assert np.array_equal(dd.cpu().numpy().view(np.uint32), want.depth[pw.HOT_AT - 100:pw.HOT_AT + 200]) and dd.max().item() >= 300
    for first, count in ((n - 99, 100), (n + 1, 0), (0, n + 1), (1 << 40, 1), (1, (1 << 64) - 1)):
        with pytest.raises(rlib.RealHipError, match="depth window") as e:
            m.pileup_depth(first, count, out=np.zeros(4, dtype=np.uint32))
        assert e.value.status == rlib.REAL_HIP_E_INVALID
    m.pileup_end()


def test_pileup_errors_are_loud_and_launch_nothing(ora, matchers):
    m, rec = matchers[1]
    w = pw.workload()
    a = _slice(w.main, 0, 200)

    def refused(word, call):
        before = m.pileup_stats()
        with pytest.raises(rlib.RealHipError, match=word) as e:
            call()
        assert e.value.status == rlib.REAL_HIP_E_INVALID
        after = m.pileup_stats()
        assert after["launches"] == before["launches"] and after["reads"] == before["reads"], word

    m.pileup_end()
    m.pileup_stats(reset=True)
    refused("add without begin", lambda: _add(m, a, rec["main"][:200]))
    refused("finish without begin", m.pileup_finish)
    refused("before finish", lambda: m.pileup_depth(0, 1))
    refused("before finish", m.pileup_sites)
    m.pileup_begin(0)
    refused("before finish", lambda: m.pileup_depth(0, 1))
    _add(m, a, rec["main"][:200])
    # more than 2^32 reads in one call: refused on the count alone (no array is looked at)
    big = rlib.RealHipBatch()
    big.struct_size, big.n_reads, big.patl = C.sizeof(rlib.RealHipBatch), (1 << 32) + 1, 50
    dummy = np.zeros(8, dtype=np.uint64)
    big.bases = dummy.ctypes.data
    refused("more than 2\\^32 reads", lambda: m._check(m._L.real_hip_pileup_add(m._h, C.byref(big), dummy.ctypes.data)))
    refused("more than 2\\^32 reads", lambda: m._check(m._L.real_hip_pileup_add_pairs(m._h, C.byref(big), C.byref(big), dummy.ctypes.data)))
    refused("min_qual", lambda: m.pileup_begin(64))
    m.pileup_finish()
    refused("add after finish", lambda: _add(m, a, rec["main"][:200]))
    refused("finish twice", m.pileup_finish)
    want = pk.Pileup(w.g.sym, 0, 0)
    want.add(a, pw.oracle_records(ora, "main", 1)[0][:200])
    assert np.array_equal(m.pileup_depth(0, want.n), want.depth)                # the refused calls changed nothing
    # the text replaced by one of another length, then by one of another file id: add is refused until the next begin
    m2 = UniqueMatcher(_opts(1))
    for fileid, sym, fs in ((0, w.g.sym[:-5], np.array([0, w.g.n - 5], dtype=np.uint64)), (3, w.g.sym, w.g.frag_start)):
        m2.set_text_symbols(0, w.g.sym, w.g.frag_start)
        m2.pileup_begin(0)
        m2.set_text_symbols(fileid, sym, fs)
        with pytest.raises(rlib.RealHipError, match="text was replaced") as e:
            _add(m2, a, rec["main"][:200])
        assert e.value.status == rlib.REAL_HIP_E_INVALID and m2.pileup_stats()["launches"] == 0
        with pytest.raises(rlib.RealHipError, match="text was replaced") as e:      # finish takes the sites' reference bases from the text
            m2.pileup_finish()
        assert e.value.status == rlib.REAL_HIP_E_INVALID and m2.pileup_stats()["launches"] == 0
    m2.pileup_begin(0)                  # (file id 3 now: every record is another file's)
    _add(m2, a, rec["main"][:200])
    assert m2.pileup_finish() == 0 and m2.pileup_stats()["other_file"] == want.stats["placed"] and m2.pileup_stats()["placed"] == 0
    m2.close()
    m.pileup_end()


@pytest.mark.parametrize("on_device", [0, 1])
def test_pileup_of_pairs(ora, on_device):
    """PairMatcher.match_pairs on the ragged pair workload (mates of 100 and 80 bases, and 60 / 120), its records asserted to
    be the pair checker's, then both mates of every Unique record piled up"""
    import torch
    g, b1, b2 = iw.workload("iid", True)
    rec, l1, l2 = iw.records(ora, "iid", True, 1)
    lo, hi = iw.WINDOW
    m = PairMatcher(RealOptions(seedl=iw.SEEDL, seedkmax=2, totalkmax=iw.TOTALK, scores=True, filter_level=iw.FILTER_LEVEL).normalise())
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    pairs = m.match_pairs(b1, b2, lo, hi)
    pc.assert_records_equal(pairs, rec, "match_pairs")
    uniq = rec["state"] == pc.UNIQUE
    assert uniq.sum() > 1000 and (l1[uniq] != l2[uniq]).sum() > 500 and (rec["inverted1"][uniq] == 1).sum() > 300
    for min_qual in (0, 10):
        want = pk.Pileup(g.sym, 0, min_qual)
        want.add_pairs(b1, b2, rec)
        assert want.stats["placed"] == 2 * int(uniq.sum()) and (want.stats["low_qual"] if min_qual else want.stats["mismatches"]) > 500
        m.pileup_stats(reset=True)
        m.pileup_begin(min_qual)
        if on_device:
            dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)]
            m.pileup_add_pairs(dev[0], dev[1], torch.from_numpy(pairs.view(np.uint8).copy()).cuda())
        else:
            m.pileup_add_pairs(b1, b2, pairs)
        _compare(m, want, 2, ("pairs", on_device, min_qual))
    m.close()


# ---- hand-made records: what no matcher writes -- placements over the text's N run, placements that end behind the text ------
def _info(state, pos, fileid=0):
    return (state << 61) | (fileid << 35) | pos


def _hand_batch(w, places, seed):
    """N-free reads that fit the text at (position, length, reverse strand): the text's own bases, but over the N run base
    x % 4 (the run is stored as A: one of four is no mismatch) and one substitution on either side of the run.  Qualities
    20..40, but 5 over the run's second position (a mismatch that is low-quality AND on an N), 40 over its third, 10 in
    front of the run and 30 behind it.  A placement that does not fit gets random bases."""
    rng = np.random.default_rng(seed)
    n, (lo, hi) = w.g.n, pw.N_RUN
    ref = np.where(w.g.sym > 3, 0, w.g.sym).astype(np.uint8)
    reads, quals = [], []
    for p, L, inv in places:
        q = rng.integers(20, 41, size=L).astype(np.uint8)
        if p + L > n:
            o = rng.integers(0, 4, size=L).astype(np.uint8)
        else:
            x = np.arange(p, p + L)
            o = ref[x].copy()
            run = (x >= lo) & (x < hi)
            o[run] = x[run] % 4
            edge = (x == lo - 1) | (x == hi)
            o[edge] = (o[edge] + 1) & 3
            q[x == lo + 1], q[x == lo + 2], q[x == lo - 1], q[x == hi] = 5, 40, 10, 30
        reads.append(synth.revcomp(o) if inv else o)
        quals.append(q[::-1] if inv else q)
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    return types.SimpleNamespace(bases=np.concatenate(reads), qual=np.concatenate(quals), offsets=off)


def _hand_places(w):
    lo, hi = pw.N_RUN
    fit = [(p, L, inv) for p in (lo - 70, lo - 31, lo - 1, lo, lo + 1, lo + 3, hi - 1, hi, hi + 1, lo - 64) for L in (33, 64, 100) for inv in (False, True)]
    beyond = [(w.g.n - 32, 33, False), (w.g.n, 40, True), (w.g.n - 99, 100, True), ((1 << 33) + 5, 50, False)]   # by one base; at n; 35 bits of position
    return fit, beyond


@pytest.mark.parametrize("min_qual", [0, 20])
@pytest.mark.parametrize("packed,on_device", [(False, 0), (True, 0), (False, 1), (True, 2)])
def test_hand_made_records_on_the_n_run_and_behind_the_text(matchers, packed, on_device, min_qual):
    m, _ = matchers[1]
    w = pw.workload()
    fit, beyond = _hand_places(w)
    places = fit[:20] + beyond[:2] + fit[20:] + beyond[2:]
    b = _hand_batch(w, places, 5)
    info = np.array([_info(2 if inv else 1, p) for p, _, inv in places], dtype=np.uint64)
    want = pk.Pileup(w.g.sym, 0, min_qual)
    want.add(b, info)
    st = want.finish_stats()
    both = sum(1 for p, L, _ in fit if p <= pw.N_RUN[0] + 1 < p + L)             # placements over the low-quality mismatch on an N
    assert st["invalid"] == len(beyond) and st["placed"] == len(fit) and st["sites"] == 2 - (1 if min_qual else 0)
    assert st["n_dropped"] > 50 and st["mismatches"] > 20 and both > 20
    if min_qual:                                                                  # quality first, then the N bit
        loose = pk.Pileup(w.g.sym, 0, 0)
        loose.add(b, info)
        assert loose.stats["n_dropped"] - st["n_dropped"] == both and st["low_qual"] > both
    m.pileup_stats(reset=True)
    m.pileup_begin(min_qual)
    _add(m, b, info, packed, on_device)
    _compare(m, want, 1, ("hand-made", packed, on_device, min_qual))
    m.pileup_end()


@pytest.mark.parametrize("on_device", [0, 1])
def test_hand_made_pairs_with_a_mate_behind_the_text(matchers, on_device):
    """pair records over the N run, one with mate 2 behind the text (mate 1 still counts), one with both"""
    import torch
    m, _ = matchers[1]
    w = pw.workload()
    n, (lo, hi) = w.g.n, pw.N_RUN
    p1 = [(lo - 60, 80, False), (lo + 2, 64, True), (n - 300, 100, False), (n - 50, 51, True), (lo - 10, 100, True), (100, 50, False)]
    p2 = [(lo - 5, 100, True), (lo + 150, 33, False), (n - 99, 100, True), (n - 10, 11, False), (lo + 40, 70, False), (300, 60, True)]
    b1, b2 = _hand_batch(w, p1, 6), _hand_batch(w, p2, 7)
    pairs = np.zeros(len(p1), dtype=rlib.PAIR_DTYPE)
    pairs["pos1"], pairs["pos2"] = [x[0] for x in p1], [x[0] for x in p2]
    pairs["inverted1"] = [int(x[2]) for x in p1]
    pairs["state"] = [pc.UNIQUE] * 5 + [pc.NONUNIQUE]
    for min_qual in (0, 20):
        want = pk.Pileup(w.g.sym, 0, min_qual)
        want.add_pairs(b1, b2, pairs)
        st = want.finish_stats()
        assert st["invalid"] == 3 and st["placed"] == 7 and st["n_dropped"] > 5 and st["reads"] == 12
        m.pileup_stats(reset=True)
        m.pileup_begin(min_qual)
        if on_device:
            dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)]
            m.pileup_add_pairs(dev[0], dev[1], torch.from_numpy(pairs.view(np.uint8).copy()).cuda())
        else:
            m.pileup_add_pairs((b1.bases, b1.qual, b1.offsets), (b2.bases, b2.qual, b2.offsets), pairs)
        _compare(m, want, 2, ("hand-made pairs", on_device, min_qual))
    m.pileup_end()


@pytest.mark.parametrize("packed,on_device", [(False, 0), (True, 1)])
def test_batch_without_qualities_counts_as_quality_30(ora, matchers, packed, on_device):
    m, rec = matchers[1]
    w = pw.workload()
    b = types.SimpleNamespace(bases=w.main.bases, qual=None, offsets=w.main.offsets)
    for min_qual in (30, 31):
        want = pk.Pileup(w.g.sym, 0, min_qual)
        want.add(b, pw.oracle_records(ora, "main", 1)[0])
        assert (want.stats["mismatches"] > 3000 and want.stats["low_qual"] == 0) if min_qual == 30 else (want.stats["mismatches"] == 0 and want.stats["low_qual"] > 3000)
        m.pileup_stats(reset=True)
        m.pileup_begin(min_qual)
        _add(m, b, rec["main"], packed, on_device)
        _compare(m, want, 1, ("no qualities", packed, on_device, min_qual))
    m.pileup_end()
