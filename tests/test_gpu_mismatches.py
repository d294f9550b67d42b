"""The mismatch lists on the device (real_hip_mismatches / _pairs) against sam_checker.py, which restates them in numpy over
the ORACLE's records.  The records handed to the library come from the matchers on the device and are first asserted to be
the oracle's / the checkers'.  Lists, offsets and statistics are integers: everything is compared exactly, and `disagree`
is 0 on every record a matcher wrote."""
import ctypes as C
import types

import numpy as np
import pytest

import pairs_checker as pc
import pairs_workloads as pairw
import pileup_workloads as pw
import sam_checker as sk
import singles_checker as sc
import singles_workloads as sw
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions, UniqueMatcher

pytestmark = pytest.mark.gpu
PAIR_CASE = sw.CASES[2]             # scores on, ragged mates (100 / 100 and 60 / 120), bucket rows


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
            info, _ = m.match_unique(b.bases, b.qual, offsets=b.offsets)
            assert np.array_equal(info, pw.oracle_records(ora, which, scores)[0]), (which, scores)
            rec[which] = info
        out[scores] = (m, rec)
    yield out
    for m, _ in out.values():
        m.close()


_want = {}


def _expected(ora, which, scores):
    """the checker's lists of a batch of the workload from the oracle's records, computed once"""
    key = (which, scores)
    if key not in _want:
        w = pw.workload()
        b = getattr(w, which)
        _want[key] = sk.mismatch_lists(w.g.sym, 0, sk.final_single(pw.oracle_records(ora, which, scores)[0]), sk.single_reads(b))
    return _want[key]


def _lists(m, b, info, packed=False, on_device=0, **kw):
    """one real_hip_mismatches of the batch in the form asked for -> (lists, offsets) as numpy"""
    import torch
    bases, nflags = (synth.pack_bases(b.bases), synth.read_nflags(b.bases, b.offsets)) if packed else (b.bases, None)
    off = b.offsets
    if on_device:
        bases, off = torch.from_numpy(bases).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        nflags = None if nflags is None else torch.from_numpy(nflags).cuda()
        if on_device == 1:
            info = torch.from_numpy(info.view(np.int64)).cuda()
    out, mo = m.mismatches(bases, None, info, offsets=off, packed=packed, nflags=nflags, **kw)
    if on_device == 1:
        out, mo = out.cpu().numpy().view(rlib.MISMATCH_DTYPE), mo.cpu().numpy().view(np.uint64)
    return out, mo


def _same(got, want, what, launches=None, m=None):
    (gl, go), (wl, wo, wst) = got, want
    assert np.array_equal(go, wo), (what, np.nonzero(go != wo)[0][:10])
    assert gl.dtype == rlib.MISMATCH_DTYPE and gl.shape == wl.shape, (what, gl.shape, wl.shape)
    for k in ("off", "ref", "base"):
        assert np.array_equal(gl[k], wl[k]), (what, k, np.nonzero(gl[k] != wl[k])[0][:10])
    if m is not None:
        st = m.mismatch_stats(reset=True)
        assert {k: st[k] for k in sk.COUNTERS} == wst, (what, st, wst)
        assert st["launches"] == launches and st["kernel_ms"] > 0, (what, st)


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("on_device", [0, 1, 2])
@pytest.mark.parametrize("packed", [False, True])
def test_lists_of_the_workload(ora, matchers, packed, on_device, scores):
    m, rec = matchers[scores]
    want = _expected(ora, "main", scores)
    assert want[2]["placed"] > 1500 and want[2]["mismatches"] > 3000 and want[2]["disagree"] == 0 and want[2]["on_n"] == 0
    m.mismatch_stats(reset=True)
    _same(_lists(m, pw.workload().main, rec["main"], packed, on_device), want, (packed, on_device, scores), 3, m)


@pytest.mark.parametrize("packed", [False, True])
def test_lists_of_long_reads(ora, matchers, packed):
    m, rec = matchers[1]
    want = _expected(ora, "long", 1)
    assert want[2]["placed"] >= 30 and want[2]["mismatches"] > 20 and want[2]["disagree"] == 0
    m.mismatch_stats(reset=True)
    _same(_lists(m, pw.workload().long, rec["long"], packed, 0), want, ("long", packed), 3, m)


def _slice(b, lo, hi):
    a, e = int(b.offsets[lo]), int(b.offsets[hi])
    return types.SimpleNamespace(bases=b.bases[a:e], offsets=(b.offsets[lo:hi + 1] - b.offsets[lo]).astype(np.uint64))


def test_two_calls_on_halves_are_one_call_on_the_whole(ora, matchers):
    m, rec = matchers[1]
    w = pw.workload()
    wl, wo, wst = _expected(ora, "main", 1)
    cut = 1111                                          # (a packed second half starts inside a byte or not: both happen below)
    for packed in (False, True):
        m.mismatch_stats(reset=True)
        l1, o1 = _lists(m, _slice(w.main, 0, cut), rec["main"][:cut], packed)
        l2, o2 = _lists(m, _slice(w.main, cut, w.main.n_reads), rec["main"][cut:], packed, 2)
        whole = (np.concatenate([l1, l2]), np.concatenate([o1, o2[1:] + o1[-1]]))
        _same(whole, (wl, wo, wst), ("halves", packed), 6, m)


def test_capacity_protocol_and_no_reads(ora, matchers):
    m, rec = matchers[1]
    w = pw.workload()
    wl, wo, wst = _expected(ora, "main", 1)
    total, n = wl.shape[0], w.main.n_reads
    b = m._read_batch(w.main.bases, None, w.main.offsets, host_records=True)
    out = np.full(total + 1, 0x07070707, dtype=np.uint32)
    off = np.zeros(n + 1, dtype=np.uint64)
    nout = C.c_uint64(0)
    call = m._L.real_hip_mismatches
    m.mismatch_stats(reset=True)
    for cap in (0, total - 1):
        assert call(m._h, C.byref(b), rec["main"].ctypes.data, out.ctypes.data, cap, C.byref(nout), off.ctypes.data) == rlib.REAL_HIP_E_OVERFLOW
        assert nout.value == total and (out == 0x07070707).all(), "nothing is written on overflow"
        st = m.mismatch_stats(reset=True)
        assert st["mismatches"] == total and st["launches"] == 2, st          # counted, not written
    assert call(m._h, C.byref(b), rec["main"].ctypes.data, out.ctypes.data, total, C.byref(nout), off.ctypes.data) == rlib.REAL_HIP_OK
    assert nout.value == total and out[-1] == 0x07070707 and np.array_equal(off, wo)
    assert np.array_equal(out[:-1].view(rlib.MISMATCH_DTYPE)["off"], wl["off"])
    _same(_lists(m, w.main, rec["main"], cap=1), (wl, wo, wst), "the mirror grows its buffer once")
    # no reads: valid, offsets[0] = 0, nothing else written
    e = m._read_batch(np.zeros(0, np.uint8), None, np.zeros(1, np.uint64), host_records=True)
    off[:] = 9
    nout.value = 5
    assert call(m._h, C.byref(e), None, None, 0, C.byref(nout), off.ctypes.data) == rlib.REAL_HIP_OK
    assert nout.value == 0 and off[0] == 0 and off[1] == 9


def test_records_of_another_file_get_empty_lists(ora, matchers):
    m, rec = matchers[1]
    w = pw.workload()
    other = pw.oracle_records(ora, "main", 1, fileid=1)[0]
    mixed = np.where(np.arange(other.shape[0]) % 3 == 0, other, rec["main"])
    want = sk.mismatch_lists(w.g.sym, 0, sk.final_single(mixed), sk.single_reads(w.main))
    assert want[2]["other_file"] > 500 and want[2]["placed"] > 1000
    m.mismatch_stats(reset=True)
    _same(_lists(m, w.main, mixed), want, "two file ids", 3, m)


# ---- pairs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [0, 1])
def test_lists_of_pairs_with_and_without_singles(ora, on_device):
    """match_pairs_singles on the ragged families workload (mates of 100 / 100 and 60 / 120 bases), its records asserted to be
    the checkers'; then the lists of the final placements with the singles and without them"""
    import torch
    w = sw.workload(ora, "families", PAIR_CASE)
    g, b1, b2, n = w["g"], w["b1"], w["b2"], w["b1"].n_reads
    scores, tk, fl, seedl, _, _, tkind, pb = PAIR_CASE
    m = PairMatcher(RealOptions(seedl=seedl, seedkmax=2, totalkmax=tk, scores=bool(scores), filter_level=fl).normalise(), prefix_bits=pb, table_kind=tkind)
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    pairs, s1, s2 = m.match_pairs_singles(b1, b2, pairw.MIN_INS, pairw.MAX_INS)
    pc.assert_records_equal(pairs, w["pairs"], "pairs")
    sc.assert_singles_equal(s1, w["s1"], "mate 1")
    sc.assert_singles_equal(s2, w["s2"], "mate 2")
    l1, l2 = w["l1"], w["l2"]
    assert (l1 != l2).sum() > 200
    dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)] if on_device else None
    up = (lambda a: torch.from_numpy(a.view(np.uint8).copy()).cuda()) if on_device else (lambda a: a)
    for given in (True, False):
        fin = sk.final_pairs(w["pairs"], w["s1"] if given else None, w["s2"] if given else None)
        want = sk.mismatch_lists(g.sym, 0, fin, sk.pair_reads(b1, b2))
        uniq = int((w["pairs"]["state"] == pc.UNIQUE).sum())
        assert want[2]["disagree"] == 0 and want[2]["mismatches"] > 1000 and want[2]["reads"] == 2 * n
        assert want[2]["placed"] > 2 * uniq + 20 if given else want[2]["placed"] == 2 * uniq
        m.mismatch_stats(reset=True)
        mates = dev if on_device else (b1, b2)
        out, mo = m.mismatches_pairs(mates[0], mates[1], up(pairs), up(s1) if given else None, up(s2) if given else None)
        if on_device:
            out, mo = out.cpu().numpy().view(rlib.MISMATCH_DTYPE), mo.cpu().numpy().view(np.uint64)
        _same((out, mo), want, ("pairs", on_device, given), 5, m)
    m.close()


# ---- hand-made records: what no matcher writes ---------------------------------------------------------------------------------
def _info(state, pos, errors=0, fileid=0):
    return (state << 61) | (errors << 41) | (fileid << 35) | pos


def _hand_batch(w, places, seed):
    """N-free reads at (position, length, reverse strand): the text's own bases, over the N run base x % 4, one substitution on
    either side of the run; a placement that does not fit gets random bases"""
    rng = np.random.default_rng(seed)
    n, (lo, hi) = w.g.n, pw.N_RUN
    ref = np.where(w.g.sym > 3, 0, w.g.sym).astype(np.uint8)
    reads = []
    for p, L, inv in places:
        if p + L > n:
            o = rng.integers(0, 4, size=L).astype(np.uint8)
        else:
            x = np.arange(p, p + L)
            o = ref[x].copy()
            run = (x >= lo) & (x < hi)
            o[run] = x[run] % 4
            edge = (x == lo - 1) | (x == hi)
            o[edge] = (o[edge] + 1) & 3
        reads.append(synth.revcomp(o) if inv else o)
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    return types.SimpleNamespace(bases=np.concatenate(reads), offsets=off)


@pytest.mark.parametrize("packed,on_device", [(False, 0), (True, 0), (False, 1), (True, 2)])
def test_hand_made_records_on_the_n_run_behind_the_text_and_with_a_wrong_count(matchers, packed, on_device):
    m, _ = matchers[1]
    w = pw.workload()
    n, (lo, hi) = w.g.n, pw.N_RUN
    fit = [(p, L, inv) for p in (lo - 70, lo - 31, lo - 1, lo, lo + 1, lo + 3, hi - 1, hi, hi + 1, lo - 64, lo - 32, n - 33, n - 64, n - 100)
           for L in (33, 64, 100) for inv in (False, True) if p + L <= n]
    beyond = [(n - 32, 33, False), (n, 40, True), (n - 99, 100, True), ((1 << 32) + 5, 50, False), ((1 << 33) + 5, 50, True)]
    places = fit[:20] + beyond[:2] + fit[20:] + beyond[2:]
    b = _hand_batch(w, places, 5)
    true_k = [0 if p + L > n else sk.placement_list(w.g.sym, b.bases[int(b.offsets[j]):int(b.offsets[j + 1])], p, inv).shape[0]
              for j, (p, L, inv) in enumerate(places)]
    assert max(true_k) <= 15
    info = np.array([_info(2 if inv else 1, p, k) for (p, _, inv), k in zip(places, true_k)], dtype=np.uint64)
    want = sk.mismatch_lists(w.g.sym, 0, sk.final_single(info), sk.single_reads(b))
    assert want[2]["invalid"] == len(beyond) and want[2]["placed"] == len(fit) and want[2]["on_n"] > 100 and want[2]["disagree"] == 0
    assert any(p + L == n for p, L, _ in fit)
    m.mismatch_stats(reset=True)
    _same(_lists(m, b, info, packed, on_device), want, ("hand-made", packed, on_device), 3, m)
    # one record whose errors field is wrong: the lists are the same, disagree is 1
    j = next(i for i, (p, L, _) in enumerate(places) if p + L <= n and true_k[i] > 0)
    wrong = info.copy()
    wrong[j] = _info(int(info[j] >> np.uint64(61)), places[j][0], true_k[j] - 1)
    want2 = sk.mismatch_lists(w.g.sym, 0, sk.final_single(wrong), sk.single_reads(b))
    assert want2[2]["disagree"] == 1 and np.array_equal(want2[1], want[1])
    _same(_lists(m, b, wrong, packed, on_device), want2, ("wrong count", packed, on_device), 3, m)


def test_hand_made_pairs_nonunique_ignores_its_singles(matchers):
    m, _ = matchers[1]
    w = pw.workload()
    n, (lo, hi) = w.g.n, pw.N_RUN
    p1 = [(lo - 60, 80, False), (lo + 2, 64, True), (n - 300, 100, False), (n - 50, 51, True), (100, 50, False), (400, 70, True), (900, 40, False)]
    p2 = [(lo - 5, 100, True), (lo + 150, 33, False), (n - 99, 100, True), (n - 10, 11, False), (300, 60, True), (700, 33, False), (1200, 90, True)]
    b1, b2 = _hand_batch(w, p1, 6), _hand_batch(w, p2, 7)
    nf = len(p1)
    pairs = np.zeros(nf, dtype=rlib.PAIR_DTYPE)
    pairs["pos1"], pairs["pos2"] = [x[0] for x in p1], [x[0] for x in p2]
    pairs["inverted1"] = [int(x[2]) for x in p1]
    pairs["state"] = [pc.UNIQUE] * 4 + [pc.NONUNIQUE, pc.NOMATCH, pc.NOMATCH]
    singles = []
    for places, states in ((p1, [1, 1, 1, 1, 1, 1, 2]), (p2, [1, 1, 1, 1, 1, 0, 1])):
        s = np.zeros(nf, dtype=rlib.SINGLE_DTYPE)
        s["pos"] = [x[0] for x in places]
        s["tag"] = [sc.make_tag(0, int(x[2]), st) for x, st in zip(places, states)]
        singles.append(s)
    for given in (True, False):
        fin = sk.final_pairs(pairs, *(singles if given else (None, None)))
        want = sk.mismatch_lists(w.g.sym, 0, fin, sk.pair_reads(b1, b2))
        # the Unique records place 8 mates, 3 of them behind the text; the NonUnique one nothing; the NoMatch ones their Unique singles
        assert want[2]["invalid"] == 3 and want[2]["placed"] == 5 + (2 if given else 0) and want[2]["reads"] == 2 * nf and want[2]["on_n"] > 5
        m.mismatch_stats(reset=True)
        got = m.mismatches_pairs((b1.bases, None, b1.offsets), (b2.bases, None, b2.offsets), pairs, *(singles if given else (None, None)))
        _same(got, want, ("hand-made pairs", given), 5, m)


def test_errors_are_loud_and_launch_nothing(matchers):
    m, rec = matchers[1]
    w = pw.workload()
    a = _slice(w.main, 0, 200)
    info = rec["main"][:200]
    b = m._read_batch(a.bases, None, a.offsets, host_records=True)
    out = np.zeros(4096, dtype=rlib.MISMATCH_DTYPE)
    off = np.zeros(401, dtype=np.uint64)
    nout = C.c_uint64(0)
    one, two = m._L.real_hip_mismatches, m._L.real_hip_mismatches_pairs
    pairs = np.zeros(200, dtype=rlib.PAIR_DTYPE)
    s = np.zeros(200, dtype=rlib.SINGLE_DTYPE)
    big = rlib.RealHipBatch()
    big.struct_size, big.n_reads, big.patl = C.sizeof(rlib.RealHipBatch), (1 << 32) + 1, 50
    big.bases = info.ctypes.data
    short = m._read_batch(a.bases[:int(a.offsets[100])], None, a.offsets[:101], host_records=True)
    dev = m._read_batch(a.bases, None, a.offsets, host_records=True)
    dev.on_device = 2
    m.mismatch_stats(reset=True)
    O, N, F, P = out.ctypes.data, C.byref(nout), off.ctypes.data, pairs.ctypes.data
    refused = [
        one(m._h, C.byref(b), info.ctypes.data, O, 4096, N, None), one(m._h, C.byref(b), info.ctypes.data, O, 4096, None, F),
        one(m._h, C.byref(b), None, O, 4096, N, F), one(m._h, C.byref(b), info.ctypes.data, None, 4096, N, F),
        one(m._h, C.byref(big), info.ctypes.data, O, 4096, N, F),
        two(m._h, C.byref(b), C.byref(b), P, s.ctypes.data, None, O, 4096, N, F), two(m._h, C.byref(b), C.byref(b), P, None, s.ctypes.data, O, 4096, N, F),
        two(m._h, C.byref(b), C.byref(short), P, None, None, O, 4096, N, F), two(m._h, C.byref(b), C.byref(dev), P, None, None, O, 4096, N, F),
        two(m._h, C.byref(b), C.byref(b), None, None, None, O, 4096, N, F), two(m._h, C.byref(big), C.byref(big), P, None, None, O, 4096, N, F),
        two(m._h, C.byref(b), C.byref(b), P, None, None, O, 4096, N, None),
    ]
    assert refused == [rlib.REAL_HIP_E_INVALID] * len(refused), refused
    st = m.mismatch_stats()
    assert st["launches"] == 0 and st["reads"] == 0, st
    bad = rlib.RealHipMismatchStats()
    bad.struct_size = 8
    assert m._L.real_hip_mismatch_stats_get(m._h, C.byref(bad), 0) == rlib.REAL_HIP_E_INVALID
    # without a text: REAL_HIP_E_STATE
    m2 = UniqueMatcher(_opts(1))
    assert m2._L.real_hip_mismatches(m2._h, C.byref(b), info.ctypes.data, O, 4096, N, F) == rlib.REAL_HIP_E_STATE
    assert m2._L.real_hip_mismatches_pairs(m2._h, C.byref(b), C.byref(b), P, None, None, O, 4096, N, F) == rlib.REAL_HIP_E_STATE
    # the text alone is enough (no index), and the context that refused still works
    m2.set_text_symbols(0, w.g.sym, w.g.frag_start)
    want = sk.mismatch_lists(w.g.sym, 0, sk.final_single(info), sk.single_reads(a))
    _same(m2.mismatches(a.bases, None, info, offsets=a.offsets), want, "text alone")
    m2.close()
    _same(m.mismatches(a.bases, None, info, offsets=a.offsets), want, "after the errors")
