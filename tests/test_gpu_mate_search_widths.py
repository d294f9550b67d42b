"""Mate search on the device at every read width and at the edges of its windows: real_hip_pair_search on the hand-made
anchors of mate_search_hand.py against mate_search_checker.search_only -- every field of every record and both FP64
values bit for bit, the four counters exactly.  The cases' own claims (states, coverage of widths, strands and roles,
window shapes) are asserted without a GPU in test_mate_search_widths_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import mate_search_checker as mc
import mate_search_hand as mh
import pairs_checker as pc
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions

pytestmark = pytest.mark.gpu

SEEDL, FL, TK = 32, 2, mh.MATRIX_TK
LIM = rlib.REAL_HIP_MATE_SEARCH_MAX_INSERT
_CASES = {}


def _cases(ora, which, scores):
    """(genome, [(bounds, fragments, batches and anchors, the checker's records, its counters)]), made once and shared"""
    if (which, scores) not in _CASES:
        g = mh.wide_genome()
        S = mc.Searcher(ora, g, SEEDL, TK, scores, *mh.MATRIX_BOUNDS)
        F = mh.matrix_cases(g, S)[0] if which == "matrix" else mh.geometry_cases(g, S, LIM)
        groups = []
        for (mn, mx), G in mh.by_bounds(F).items():
            B = mh.batches(G)
            b1, b2, (h1, o1), (h2, o2) = B
            want, ctr = mc.search_only(ora, {0: g}, [(0, h1, o1, h2, o2)], b1, b2, mn, mx, scores, ora.filter_mult(FL, TK), SEEDL, TK)
            assert [int(s) for s in want["state"]] == [f.state for f in G]
            want.setflags(write=False)
            groups.append(((mn, mx), G, B, want, ctr))
        _CASES[(which, scores)] = (g, groups)
    return _CASES[(which, scores)]


def _packed_batch(b, lead):
    """2-bit packed bases with nflags; ``lead`` bases in front of everything, so that reads start inside a byte"""
    packed = synth.pack_bases(np.concatenate([np.zeros(lead, np.uint8), b.bases]))
    qual = np.concatenate([np.zeros(lead, np.uint8), b.qual])
    flags, offs = synth.read_nflags(b.bases, b.offsets), (b.offsets + np.uint64(lead)).astype(np.uint64)
    rb = rlib.RealHipBatch()
    rb.struct_size, rb.on_device, rb.n_reads = C.sizeof(rlib.RealHipBatch), 0, b.n_reads
    rb.bases, rb.qual, rb.offsets, rb.packed, rb.nflags, rb.fresh = packed.ctypes.data, qual.ctypes.data, offs.ctypes.data, 1, flags.ctypes.data, 1
    rb._keep = (packed, qual, flags, offs)
    return rb


def _differing(got, want):
    return [i for i in range(len(want)) if any(np.asarray(got[f][i]).tobytes() != np.asarray(want[f][i]).tobytes() for f in pc.FIELDS)]


def _counters(st):
    return {k: st[k] for k in mc.COUNTERS}


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("which", ["matrix", "geometry"])
def test_pair_search_widths_and_window_edges(ora, which, scores):
    g, groups = _cases(ora, which, scores)
    m = PairMatcher(RealOptions(seedl=SEEDL, seedkmax=2, totalkmax=TK, scores=bool(scores), filter_level=FL).normalise())
    m.set_text_symbols(0, g.sym, g.frag_start)                       # the search needs the text, not the index
    for (mn, mx), G, (b1, b2, (h1, o1), (h2, o2)), want, ctr in groups:
        what = "%s, inserts %d..%d" % (which, mn, mx)
        p1, p2 = mh.product_hits(h1, rlib.HIT_DTYPE), mh.product_hits(h2, rlib.HIT_DTYPE)
        m.mate_search_stats(reset=True)
        got = m.pair_search(b1, b2, p1, o1, p2, o2, mn, mx)
        wrong = [G[i].what for i in _differing(got, want)]
        pc.assert_records_equal(got, want, "%s, byte bases %r" % (what, wrong[:5]))
        assert _counters(m.mate_search_stats(reset=True)) == ctr, what
        # 2-bit packed bases with nflags, reads starting inside a byte: the same records
        bb1, bb2 = _packed_batch(b1, 1), _packed_batch(b2, 3)
        out = PairMatcher.new_pair_info(len(G))
        pp, sp = m._pair_params(mn, mx), m._search_params(0)
        m._check(m._L.real_hip_pair_search(m._h, C.byref(pp), C.byref(sp), C.byref(bb1), C.byref(bb2), p1.ctypes.data, o1.ctypes.data,
                                           p2.ctypes.data, o2.ctypes.data, 0, 1, out.ctypes.data))
        pc.assert_records_equal(out, want, "%s, packed bases %r" % (what, [G[i].what for i in _differing(out, want)][:5]))
        pc.assert_records_equal(out, got, what + ", packed against byte bases")
        assert _counters(m.mate_search_stats(reset=True)) == ctr, what + ", packed"
    m.close()
