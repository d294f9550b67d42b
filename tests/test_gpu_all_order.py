"""real_hip_match_all's ordering pass (real_amd/csrc/all_order.hip) at the edges of its three paths, against the oracle, bit for
bit: reads with 0, 1, 2 .. 32, 33 .. 1024 and more hits on both sides of every threshold, strand ties behind the radix sort,
hit lists spread over many k, the second trip of the lane grid and of the workgroups, a hit buffer of exactly the hits' size,
and the state the pass leaves for the next call (all_order_workloads.py; test_all_order_cpu.py shows what the batches hold)."""
import ctypes as C

import numpy as np
import pytest

import all_order_workloads as aw
from real_amd import lib as rlib
from real_amd.matcher import AllMatcher, RealOptions

pytestmark = pytest.mark.gpu

# seedl, prefix_bits, table_kind asked, layout built (left to itself a 16-base index of this size gets digest directories)
GEOMETRY = {"starts": (aw.SEEDL, 0, 1, rlib.LAYOUT_STARTS), "rows": (aw.SEEDL, 13, 3, rlib.LAYOUT_ROWS)}
WORK = ("reads", "lookups", "candidates", "seedpass", "hits")


def _new(geometry):
    w = aw.workload()
    seedl, pb, tk, built = GEOMETRY[geometry]
    m = AllMatcher(RealOptions(seedl=seedl, seedkmax=aw.SEEDKMAX, totalkmax=aw.K, scores=True).normalise(), prefix_bits=pb, table_kind=tk)
    m.set_text_symbols(0, w.g.sym, w.g.frag_start)
    m.build_index_block()
    assert m.table_kind == built, m.table_kind
    return m


@pytest.fixture(scope="module")
def matchers():
    import torch
    torch.zeros(1, device="cuda")       # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    out = {}

    def get(geometry):
        if geometry not in out:
            out[geometry] = _new(geometry)
        return out[geometry]
    yield get
    for m in out.values():
        m.close()


def _all(m, b, where, cap, offsets=True):
    """real_hip_match_all through the C ABI, host or device arrays, once -> (status, n_out, hits[:cap], offsets or None)"""
    import torch
    n = b.n_reads
    nout = C.c_uint64(0)
    if where == "host":
        batch = m._read_batch(b.bases, b.qual, b.offsets)
        hits, hoff = np.zeros(cap, dtype=rlib.HIT_DTYPE), np.zeros(n + 1, dtype=np.uint64)
        rc = m._L.real_hip_match_all(m._h, C.byref(batch), hits.ctypes.data, cap, C.byref(nout), hoff.ctypes.data if offsets else None)
    else:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        batch = m._read_batch(up(b.bases), up(b.qual), up(b.offsets.view(np.int64)))
        dh, do = torch.zeros((cap, 4), dtype=torch.int32, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        m.sync_inputs(dh, do)
        rc = m._L.real_hip_match_all(m._h, C.byref(batch), dh.data_ptr(), cap, C.byref(nout), do.data_ptr() if offsets else None)
        hits, hoff = dh.cpu().numpy().view(rlib.HIT_DTYPE).reshape(-1), do.cpu().numpy().view(np.uint64)
    return rc, int(nout.value), hits, hoff if offsets else None


def _same(hits, hoff, o, what):
    """the library's records against the oracle's, field by field, the scores as bits; hoff = None: the hits alone"""
    assert hoff is None or np.array_equal(hoff, o.hoff), (what, np.nonzero(hoff != o.hoff)[0][:10])
    assert hits.shape[0] == o.hits.shape[0], (what, hits.shape, o.hits.shape)
    for f in ("read", "pos", "frag", "k", "inverted"):
        bad = np.nonzero(hits[f].astype(np.uint64) != o.hits[f].astype(np.uint64))[0]
        assert bad.size == 0, (what, f, bad[:10], hits[bad[:4]], o.hits[bad[:4]])
    bad = np.nonzero(hits["score"].view(np.uint32) != o.hits["score"].view(np.uint32))[0]
    assert bad.size == 0, (what, "score bits", bad[:10])


def _run(m, ora, name, scores, where="host", offsets=True, slack=0):
    """one call with a hit buffer of the oracle's total (+ slack): status, count, records, offsets and work counters"""
    o = aw.oracle(ora, name, scores)
    total = int(o.hits.shape[0])
    m.set_match_params(totalkmax=aw.TOTALKMAX[name], scores=bool(scores))
    m.counters(reset=True)
    rc, nout, hits, hoff = _all(m, aw.batch_of(name), where, total + slack, offsets)
    what = (name, scores, where, offsets)
    assert rc == 0 and nout == total, (what, rc, nout, total)
    _same(hits[:nout], hoff, o, what)
    c = m.counters(reset=True)
    assert {k: c[k] for k in WORK} == {k: o.ctr[k] for k in WORK}, (what, c, o.ctr)
    return hits[:nout], hoff


@pytest.mark.parametrize("geometry", ["starts", "rows"])
def test_edges_and_spread_with_a_hit_buffer_of_exactly_the_hits(ora, geometry):
    """A context of its own, the smaller batch first: the raw buffer only grows, so in each of these calls it is exactly
    n_raw records long and the last read's radix scratch (the last read of `edges` has more than 1024 hits) ends at its end."""
    m = _new(geometry)
    try:
        assert aw.oracle(ora, "spread").hits.shape[0] < aw.oracle(ora, "edges").hits.shape[0]
        for name in ("spread", "edges"):
            for scores in (1, 0):
                for where in ("host", "device"):
                    _run(m, ora, name, scores, where)
                    _run(m, ora, name, scores, where, offsets=False)
    finally:
        m.close()


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("geometry", ["starts", "rows"])
def test_an_overflow_then_the_same_context(ora, matchers, geometry, scores):
    m = matchers(geometry)
    for name in ("edges", "spread"):
        o = aw.oracle(ora, name, scores)
        total = int(o.hits.shape[0])
        m.set_match_params(totalkmax=aw.TOTALKMAX[name], scores=bool(scores))
        for where in ("host", "device"):
            rc, nout, _, _ = _all(m, aw.batch_of(name), where, total - 1)
            assert rc == rlib.REAL_HIP_E_OVERFLOW and nout == total, (name, where, rc, nout, total)
            _run(m, ora, name, scores, where)


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("geometry", ["starts", "rows"])
def test_the_state_between_calls(ora, matchers, geometry, scores):
    """cursor[] and the two counters are the pass's own between calls: batches with other sets of multi-hit reads, other read
    counts and other totals one after the other on one context"""
    m = matchers(geometry)
    for i, name in enumerate(("edges", "edges_permuted", "edges", "spread", "edges_permuted")):
        _run(m, ora, name, scores, "device" if i % 2 else "host", slack=(0, 8, 0)[i % 3])


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("geometry", ["starts", "rows"])
def test_the_same_call_twice(ora, matchers, geometry, scores):
    """the scatter takes its slots by atomics: the raw order may differ from call to call, the output may not"""
    m = matchers(geometry)
    for where in ("host", "device"):
        h1, o1 = _run(m, ora, "edges", scores, where)
        h2, o2 = _run(m, ora, "edges", scores, where)
        assert h1.tobytes() == h2.tobytes() and o1.tobytes() == o2.tobytes()


@pytest.mark.parametrize("geometry", ["starts", "rows"])
def test_every_workgroup_takes_a_second_read(ora, matchers, geometry):
    """many_big: 1140 reads with more than 32 hits for 1024 workgroups, 40 of them radix reads among the quadratic ones"""
    o = aw.oracle(ora, "many_big", 1)
    c = np.diff(o.hoff.astype(np.int64))
    assert (c > 32).sum() == 1140 and (c > 1024).sum() == 40
    _run(matchers(geometry), ora, "many_big", 1)


def test_the_lane_grid_takes_a_second_trip(ora, matchers):
    """many_multi: 528 384 reads with two hits or more for 2048 x 256 lanes; the expectation is the oracle's answer for the
    three distinct reads, tiled (test_all_order_cpu.py compares it with the oracle on the first 4096 reads)"""
    o = aw.oracle(ora, "many_multi", 1)
    assert (np.diff(o.hoff.astype(np.int64)) >= 2).sum() - 2048 * 256 >= 16 * 256
    _run(matchers("starts"), ora, "many_multi", 1)
