"""The hand-made cases of test_gpu_mate_search_widths.py hold what they claim, on the checker's records alone (no GPU):
the states their construction means, every width with both strands and both anchor roles, the forced substitution
places, the differing base behind the k = totalkmax placements, and the window shapes of the geometry cases."""
import numpy as np
import pytest

import mate_search_checker as mc
import mate_search_hand as mh
import pairs_checker as pc
from real_amd import lib as rlib

SEEDL, FL = 32, 2
LIM = rlib.REAL_HIP_MATE_SEARCH_MAX_INSERT


def _records(ora, g, F, scores, tk=mh.MATRIX_TK):
    """the checker's records of the fragments, group by group, in the order of F"""
    out, where = np.zeros(len(F), dtype=pc.REC_DTYPE), {id(f): i for i, f in enumerate(F)}
    for (mn, mx), G in mh.by_bounds(F).items():
        b1, b2, (h1, o1), (h2, o2) = mh.batches(G)
        want, _ = mc.search_only(ora, {0: g}, [(0, h1, o1, h2, o2)], b1, b2, mn, mx, scores, ora.filter_mult(FL, tk), SEEDL, tk)
        for f, r in zip(G, want):
            out[where[id(f)]] = r
    return out


def _assert_states(F, want):
    wrong = [(f.what, int(s)) for f, s in zip(F, want["state"]) if int(s) != f.state]
    assert not wrong, wrong


@pytest.mark.parametrize("scores", [1, 0])
def test_the_length_matrix_covers_every_width(ora, scores):
    g = mh.wide_genome()
    assert g.n % 32 and g.n % 64 and g.n_frag == 2 and 0 < (g.sym > 3).sum() < 8
    tk = mh.MATRIX_TK
    S = mc.Searcher(ora, g, SEEDL, tk, scores, *mh.MATRIX_BOUNDS)
    F, cells = mh.matrix_cases(g, S)
    assert 200 <= len(F) == len(cells) == len(mh.LA_SET) * len(mh.LB_SET) * 9 <= 600
    want = _records(ora, g, F, scores)
    _assert_states(F, want)
    for lb in mh.LB_SET:
        mine = [(c, r) for c, r in zip(cells, want) if c.lb == lb]
        for k, state in ((0, pc.UNIQUE), (tk, pc.UNIQUE), (tk + 1, pc.NOMATCH)):
            rows = [(c, r) for c, r in mine if c.k == k]
            assert len(rows) == 9 and all(r["state"] == state for _, r in rows), (lb, k)
            assert {c.la for c, _ in rows} == set(mh.LA_SET) and {c.align for c, _ in rows} == set(mh.ALIGN_SET)
        assert {(c.role, c.inva) for c, _ in mine} == set(mh.ANCHOR_COMBOS), lb
    for W in range(1, 11):                                           # every width: both strands and both anchor roles, found and refused
        mine = [c for c in cells if (c.lb + 31) // 32 == W]
        for k in (0, tk, tk + 1):
            assert {(c.role, c.inva) for c in mine if c.k == k} == set(mh.ANCHOR_COMBOS), (W, k)
    for c, r in zip(cells, want):
        assert c.p % 32 == c.align and len(c.at) == c.k
        if r["state"] == pc.UNIQUE:
            assert int(r["k2"] if c.role == 0 else r["k1"]) == c.k and int(r["pos2"] if c.role == 0 else r["pos1"]) == c.p
        if c.k:
            assert c.lb - 1 in c.at and 0 in c.at, "a substitution at the last base and at the first"
        if c.k and c.lb > 32:
            assert any(x % 32 in (0, 31) and 0 < x < c.lb - 1 for x in c.at), "a substitution beside a word boundary"
        if c.k == tk + 1 and c.lb > 33:
            assert any(x % 32 == 31 and x + 1 in c.at for x in c.at), "both sides of one word boundary"
        if c.k == tk:                                                # a compare that runs one base too far counts tk + 1
            assert g.sym[c.p + c.lb] in (1, 2, 3)
    last = {(c.lb + 31) // 32 for c in cells if c.k and c.lb > 32 and any(x in c.at for x in (32 * ((c.lb - 1) // 32) - 1, 32 * ((c.lb - 1) // 32)))}
    assert last == set(range(2, 11)), "the boundary in front of the last word, at every width"
    both = [r for c, r in zip(cells, want) if r["state"] == pc.UNIQUE]
    assert {int(r["inverted1"]) for r in both} == {0, 1}


def test_the_geometry_cases_are_what_they_say(ora):
    g = mh.wide_genome()
    tk = mh.MATRIX_TK
    S = mc.Searcher(ora, g, SEEDL, tk, 1, *mh.MATRIX_BOUNDS)
    F = mh.geometry_cases(g, S, LIM)
    _assert_states(F, _records(ora, g, F, 1))
    assert len({f.what for f in F}) == len(F)
    fs = [int(v) for v in g.frag_start]
    seen = set()
    for f in F:                                                      # the windows, from the anchors alone
        for m, hits in enumerate((f.a1, f.a2)):
            la, lb = (len(f.r1), len(f.r2)) if m == 0 else (len(f.r2), len(f.r1))
            for pa, frag, inv, _, _ in hits:
                lo, hi = mc.window_of(pa, la, lb, inv, fs[frag], fs[frag + 1], *f.bounds)
                words = ((hi + lb - 1) >> 5) - (lo >> 5) + 2         # text words the window needs, one more for the funnel shift
                assert words <= LIM // 32 + 2
                if f.bounds[1] == LIM and hi - lo + lb == LIM:
                    seen.add((lb, inv, lo % 32, words))
    for lb in (320, 32):
        for inv in (0, 1):
            assert (lb, inv, 31, LIM // 32 + 2) in seen, "a full window at lo = 31 mod 32 needs every word of the LDS region"
            assert (lb, inv, 0, LIM // 32 + 1) in seen
    assert (320, 0, 1, LIM // 32 + 2) in seen and (320, 1, 1, LIM // 32 + 2) in seen
    spans = {f.bounds[1] - f.bounds[0] + 1 for f in F if f.what.startswith("window of")}
    assert {s % 64 for s in spans} == {0, 1, 63}
