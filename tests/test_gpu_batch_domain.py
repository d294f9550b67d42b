"""The matcher at the edges of the batch domain (domain_workloads.py) against the oracle, bit for bit: reads of 0 .. 16384
bases on both sides of every threshold of the lane and the wave kernel, quality bytes 0..127, reads without bases; info words,
score bits, hit lists and work counters, in every form a batch can take.  Then the pair joins on the workload's mates and the
refusal of a 16385-base read."""
import ctypes as C

import numpy as np
import pytest

import domain_workloads as dw
import pairs_all_checker as pac
import pairs_checker as pc
import pairs_workloads as pw
import singles_checker as sc
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions, new_unique_info

pytestmark = pytest.mark.gpu

GEOMETRY = {"starts": (32, 0, 0), "rows": (16, 13, 3)}          # seedl, prefix_bits, table_kind
WORK = ("reads", "lookups", "candidates", "seedpass", "hits")
WIDE_INS = 17_000                                               # an outer distance that holds a 16384-base mate


@pytest.fixture(scope="module")
def matchers():
    import torch
    torch.zeros(1, device="cuda")       # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    w = dw.workload()
    out = {}

    def get(geometry):
        if geometry not in out:
            seedl, pb, tk = GEOMETRY[geometry]
            m = PairMatcher(RealOptions(seedl=seedl, seedkmax=dw.SEEDKMAX, totalkmax=dw.TOTALKMAX, scores=True).normalise(), prefix_bits=pb, table_kind=tk)
            m.set_text_symbols(0, w.g.sym, w.g.frag_start)
            m.build_index_block()
            if geometry == "rows":
                assert m.table_kind == rlib.LAYOUT_ROWS, m.table_kind
            out[geometry] = m
        return out[geometry]
    yield get
    for m in out.values():
        m.close()


def _forms(b, qual, packed, where):
    """the arrays of batch b in the form asked for -> (bases, qual, offsets, nflags, keyword arguments)"""
    import torch
    bases, nflags = (synth.pack_bases(b.bases), synth.read_nflags(b.bases, b.offsets)) if packed else (b.bases, None)
    off = b.offsets
    kw = dict(packed=packed)
    if where != "host":
        # (an array without elements: a valid address of which nothing is read -- an empty tensor has the address 0, and a NULL
        # `bases` with n_reads > 0 is an argument error)
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() if a.size else torch.zeros(16, dtype=torch.uint8, device="cuda")
        bases, qual, nflags, off = up(bases), up(qual), up(nflags), up(off.view(np.int64))
        if where == "declared":
            kw["max_patl"] = rlib.REAL_HIP_MAX_PATL_LONG
    return bases, qual, off, nflags, kw


def _unique(m, b, qual, packed, where):
    """real_hip_match_unique -> (info, score bits or None) as numpy"""
    import torch
    bases, q, off, nflags, kw = _forms(b, qual, packed, where)
    n = b.n_reads
    if where == "host":
        info, score = m.match_unique(bases, q, off, nflags=nflags, **kw)
    else:
        i0, s0 = new_unique_info(n, m.opts.scores)
        info = torch.from_numpy(i0.view(np.int64)).cuda()
        score = None if s0 is None else torch.from_numpy(s0).cuda()
        m.match_unique(bases, q, off, info=info, score=score, nflags=nflags, **kw)
        info, score = info.cpu().numpy().view(np.uint64), None if score is None else score.cpu().numpy()
    return info, None if score is None else score.view(np.uint32)


def _all(m, b, qual, packed, where, cap):
    """real_hip_match_all through the C ABI in the form asked for -> (hits, offsets) as numpy"""
    import torch
    bases, q, off, nflags, kw = _forms(b, qual, packed, where)
    n = b.n_reads
    batch = m._read_batch(bases, q, off, nflags=nflags, **kw)
    nout = C.c_uint64(0)
    if where == "host":
        hits, hoff = np.zeros(cap, dtype=rlib.HIT_DTYPE), np.zeros(n + 1, dtype=np.uint64)
        m._check(m._L.real_hip_match_all(m._h, C.byref(batch), hits.ctypes.data, cap, C.byref(nout), hoff.ctypes.data))
    else:
        dh, do = torch.zeros((cap, 4), dtype=torch.int32, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        m.sync_inputs(dh, do)
        m._check(m._L.real_hip_match_all(m._h, C.byref(batch), dh.data_ptr(), cap, C.byref(nout), do.data_ptr()))
        hits, hoff = dh.cpu().numpy().view(rlib.HIT_DTYPE).reshape(-1), do.cpu().numpy().view(np.uint64)
    return hits[:int(nout.value)], hoff


def _same_hits(got, want, what):
    (gh, go), (wh, wo) = got, want
    assert np.array_equal(go, wo), (what, np.nonzero(go != wo)[0][:10])
    assert gh.shape[0] == wh.shape[0], (what, gh.shape, wh.shape)
    for k in ("pos", "k", "inverted", "frag"):
        assert np.array_equal(gh[k], wh[k]), (what, k, np.nonzero(gh[k] != wh[k])[0][:10])
    assert np.array_equal(gh["score"].view(np.uint32), wh["score"].view(np.uint32)), (what, "score bits")
    assert np.array_equal(gh["read"].astype(np.uint64), wh["read"]), (what, "read")


def _check(m, ora, which, seedl, scores, qual, packed, where):
    w = dw.workload()
    b = dw.batch_of(w, which)
    o = dw.oracle(ora, which, seedl, scores, qual)
    what = (which, seedl, scores, qual, packed, where)
    m.set_match_params(scores=bool(scores))
    m.counters(reset=True)
    info, bits = _unique(m, b, b.qual if qual else None, packed, where)
    bad = np.nonzero(info != o.info)[0]
    assert bad.size == 0, (what, [(int(i), w.meta[i] if which in ("b", "b63") else None, hex(int(info[i])), hex(int(o.info[i]))) for i in bad[:5]])
    if scores:
        bad = np.nonzero(bits != o.score.view(np.uint32))[0]
        assert bad.size == 0, (what, [(int(i), w.meta[i] if which in ("b", "b63") else None) for i in bad[:5]])
    c = m.counters(reset=True)
    assert {k: c[k] for k in WORK} == {k: o.ctr[k] for k in WORK}, (what, c, o.ctr)
    long = dw.lens_of(b) > rlib.REAL_HIP_MAX_PATL
    if which not in ("b", "b63"):       # (a batch of long reads only: one with an N is not eligible and need not be handed over)
        long = long & ~np.array([(b.bases[int(b.offsets[i]):int(b.offsets[i + 1])] > 3).any() for i in range(b.n_reads)], dtype=bool)
    assert c["handed_over"] >= int(long.sum()), (what, c["handed_over"], int(long.sum()))
    got = _all(m, b, b.qual if qual else None, packed, where, o.hits.shape[0] + 8)
    _same_hits(got, (o.hits, o.hoff), what)
    c = m.counters(reset=True)
    assert {k: c[k] for k in WORK} == {k: o.actr[k] for k in WORK}, (what, c, o.actr)
    return o


@pytest.mark.parametrize("where", ["host", "device", "declared"])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("geometry", ["starts", "rows"])
def test_the_ragged_batch_against_the_oracle(ora, matchers, geometry, scores, packed, where):
    _check(matchers(geometry), ora, "b", GEOMETRY[geometry][0], scores, True, packed, where)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("geometry", ["starts", "rows"])
def test_the_twin_with_qualities_below_64(ora, matchers, geometry, scores, packed):
    _check(matchers(geometry), ora, "b63", GEOMETRY[geometry][0], scores, True, packed, "host")


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("geometry", ["starts", "rows"])
def test_the_batch_without_qualities(ora, matchers, geometry, where):
    """qual = NULL: every base counts as quality 30 (Pattern.hpp:42-45), beyond WV_QL bases as below it"""
    _check(matchers(geometry), ora, "b", GEOMETRY[geometry][0], 1, False, False, where)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("patl", dw.UNIFORM)
def test_uniform_batches_at_the_thresholds(ora, matchers, patl, packed):
    """offsets = NULL: every read of the batch has `patl` bases (a packed read then starts inside a byte when patl is odd)"""
    import torch
    m = matchers("starts")
    w = dw.workload()
    b = w.uniform[patl]
    n = b.n_reads
    for scores in (1, 0):
        o = dw.oracle(ora, patl, 32, scores)
        m.set_match_params(scores=bool(scores))
        bases, nflags = (synth.pack_bases(b.bases), synth.read_nflags(b.bases, b.offsets)) if packed else (b.bases, None)
        m.counters(reset=True)
        info, score = m.match_unique(bases, b.qual, None, patl=patl, n_reads=n, packed=packed, nflags=nflags)
        assert np.array_equal(info, o.info), (patl, packed, scores)
        assert not scores or np.array_equal(score.view(np.uint32), o.score.view(np.uint32)), (patl, packed, scores)
        c = m.counters(reset=True)
        assert {k: c[k] for k in WORK} == {k: o.ctr[k] for k in WORK} and c["handed_over"] >= n - 1, (c, o.ctr)      # (one read holds an N)
        up = lambda a: None if a is None else torch.from_numpy(a).cuda()
        i0, s0 = new_unique_info(n, bool(scores))
        di, ds = up(i0.view(np.int64)), up(s0)
        m.match_unique(up(bases), up(b.qual), None, patl=patl, n_reads=n, info=di, score=ds, packed=packed, nflags=up(nflags))
        assert np.array_equal(di.cpu().numpy().view(np.uint64), o.info), (patl, packed, scores, "device")
        assert not scores or np.array_equal(ds.cpu().numpy().view(np.uint32), o.score.view(np.uint32))
        if not packed:
            hits, hoff = m.match_all(b.bases, b.qual, None, patl=patl, n_reads=n)
            _same_hits((hits, hoff), (o.hits, o.hoff), (patl, scores))
    assert ((dw.oracle(ora, patl, 32, 1).info >> np.uint64(61)) == 1).sum() >= 4


@pytest.mark.parametrize("where", ["host", "device", "declared"])
@pytest.mark.parametrize("which", ["empty", "edge_empty"])
def test_reads_without_bases(ora, matchers, which, where):
    """a batch of reads without bases only (n_reads > 0, zero bases in all: no error, nothing placed, no hit), and a batch whose
    first and last read are empty"""
    for packed in (False, True):
        o = _check(matchers("starts"), ora, which, 32, 1, True, packed, where)
        assert o.info[0] == 0 and o.info[-1] == 0
    if which == "empty":
        assert not o.info.any() and o.hits.shape[0] == 0 and o.ctr["reads"] == 0


# ---- pairs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_ins", [pw.MAX_INS, WIDE_INS])
@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("geometry", ["starts", "rows"])
def test_the_pair_joins_on_mates_at_the_edges(ora, matchers, geometry, scores, max_ins):
    """mates of (2049, 100), (100, 16384), (0, 100) and (100, 31) bases: match_pairs, match_pairs_all and match_pairs_singles
    against the checkers on the oracle's lists.  Inside the insert bounds of pairs_workloads.py only the short fragments can
    be concordant; the wide bound lets the long mates pair as well."""
    w = dw.workload()
    b1, b2 = w.pairs
    seedl = GEOMETRY[geometry][0]
    o1, o2 = dw.oracle(ora, "pairs1", seedl, scores), dw.oracle(ora, "pairs2", seedl, scores)
    f = (0, o1.hits, o1.hoff, o2.hits, o2.hoff)
    l1, l2 = pw.lens_of(b1), pw.lens_of(b2)
    fm = ora.filter_mult(2, dw.TOTALKMAX)
    want = pc.check_pairs([f], l1, l2, pw.MIN_INS, max_ins, scores, fm)
    uniq = want["state"] == pc.UNIQUE
    long_mate = (np.maximum(l1, l2) > 2000)
    assert (uniq & long_mate).sum() == (6 if max_ins == WIDE_INS else 0), (want["state"], long_mate)
    assert not uniq[(l1 == 0) | (l2 == 0)].any() and (seedl == 16 or not uniq[(l1 == 31) | (l2 == 31)].any())
    m = matchers(geometry)
    m.set_match_params(scores=bool(scores))
    got = m.match_pairs(b1, b2, pw.MIN_INS, max_ins)
    pc.assert_records_equal(got, want, "match_pairs")
    wa, woff = pac.enumerate_pairs(o1.hits, o1.hoff, l1, o2.hits, o2.hoff, l2, pw.MIN_INS, max_ins, 0)
    ga, goff = m.match_pairs_all(b1, b2, pw.MIN_INS, max_ins)
    np.testing.assert_array_equal(goff, woff)
    pac.assert_pair_hits_equal(ga, wa, "match_pairs_all")
    s1 = sc.check_singles([(0, o1.hits, o1.hoff)], l1, scores, fm)
    s2 = sc.check_singles([(0, o2.hits, o2.hoff)], l2, scores, fm)
    gp, g1, g2 = m.match_pairs_singles(b1, b2, pw.MIN_INS, max_ins)
    pc.assert_records_equal(gp, want, "match_pairs_singles")
    sc.assert_singles_equal(g1, s1, "mate 1")
    sc.assert_singles_equal(g2, s2, "mate 2")
    assert (sc.state_of(s2["tag"])[l2 == 16384] == 1).all() and (sc.state_of(s1["tag"])[l1 == 0] == 0).all()


def test_the_mate_search_refuses_a_mate_of_321_bases(matchers):
    w = dw.workload()
    m = matchers("starts")
    with pytest.raises(rlib.RealHipError) as e:
        m.match_pairs(w.pairs[0], w.pairs[1], pw.MIN_INS, pw.MAX_INS, mate_search=True)
    assert e.value.status == rlib.REAL_HIP_E_UNSUPPORTED


# ---- one base too many ---------------------------------------------------------------------------------------------------
def _too_long(alone):
    """a read of 16385 bases, alone or behind four good 100-base reads of the workload"""
    w = dw.workload()
    good = dw.subset(w.b, [] if alone else [i for i, x in enumerate(w.meta) if x[1] == "fill"][:4])
    r = w.g.sym[dw.P_MID:dw.P_MID + 16385].copy()
    bases = np.concatenate([good.bases, r])
    qual = np.concatenate([good.qual, np.full(16385, 40, np.uint8)])
    off = np.concatenate([good.offsets, [good.offsets[-1] + 16385]]).astype(np.uint64)
    return bases, qual, off


@pytest.mark.parametrize("alone", [True, False])
@pytest.mark.parametrize("where,status", [("host", rlib.REAL_HIP_E_UNSUPPORTED), ("device", rlib.REAL_HIP_E_UNSUPPORTED),
                                          ("declared", rlib.REAL_HIP_E_INVALID)])
def test_a_read_of_16385_bases_is_refused(ora, matchers, where, status, alone):
    """Host arrays, and device arrays whose lengths the library measures itself (max_patl = 0): REAL_HIP_E_UNSUPPORTED before
    anything is launched, every record stays as it was.  Device offsets with a declared max_patl: the kernel meets the read,
    REAL_HIP_E_INVALID; the read's own record stays as it was (include/real_hip.h says nothing of its neighbours' after a
    failed call: the lane matcher has by then written some of them).  The next good call is the oracle's."""
    import torch
    m = matchers("starts")
    m.set_match_params(scores=True)
    bases, qual, off = _too_long(alone)
    n = off.shape[0] - 1
    i0 = np.full(n, 0x1234, dtype=np.uint64)
    s0 = np.full(n, 7.0, dtype=np.float32)
    if where == "host":
        info, score = i0.copy(), s0.copy()
        args = (bases, qual, off)
        kw = {}
    else:
        info, score = torch.from_numpy(i0.view(np.int64).copy()).cuda(), torch.from_numpy(s0.copy()).cuda()
        args = (torch.from_numpy(bases).cuda(), torch.from_numpy(qual).cuda(), torch.from_numpy(off.view(np.int64)).cuda())
        kw = dict(max_patl=rlib.REAL_HIP_MAX_PATL_LONG) if where == "declared" else {}
    with pytest.raises(rlib.RealHipError) as e:
        m.match_unique(*args, info=info, score=score, **kw)
    assert e.value.status == status, (e.value.status, str(e.value))
    if where != "host":
        info, score = info.cpu().numpy().view(np.uint64), score.cpu().numpy()
    keep = slice(n - 1, n) if where == "declared" else slice(0, n)
    assert np.array_equal(info[keep], i0[keep]) and np.array_equal(score[keep], s0[keep]), "the records are untouched"
    with pytest.raises(rlib.RealHipError) as e:
        m.match_all(bases, qual, off)
    assert e.value.status == rlib.REAL_HIP_E_UNSUPPORTED
    _check(m, ora, 16384, 32, 1, True, False, "host" if where == "host" else "device")
