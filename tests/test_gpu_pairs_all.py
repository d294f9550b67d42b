"""Every concordant pair of a fragment on the device (real_hip_pair_all_hits / real_hip_match_pairs_all) against the
brute-force checker of pairs_all_checker.py, which walks the product row-major with pairs_checker.concordant and never
calls the code under test."""
import ctypes as C

import numpy as np
import pytest

import pairs_all_checker as pac
import pairs_workloads as pw
from real_amd import lib as rlib
from real_amd.matcher import PairMatcher, RealOptions

pytestmark = pytest.mark.gpu

MIN_INS, MAX_INS = 150, 420


def _opts(seedl, totalkmax, scores, filter_level):
    return RealOptions(seedl=seedl, seedkmax=2, totalkmax=totalkmax, scores=bool(scores), filter_level=filter_level).normalise()


# ---- the enumeration alone, on hand-made lists ----------------------------------------------------------------------
def _hits(rows):
    h = np.zeros(len(rows), dtype=rlib.HIT_DTYPE)
    for j, (pos, frag, inv, k, score) in enumerate(rows):
        h[j] = (0, pos, score, frag, k, inv)
    return h


def _lists(frags):
    """frags: [(rows of mate 1, rows of mate 2, len1, len2)] -> hits1, off1, len1, hits2, off2, len2"""
    o1 = np.cumsum([0] + [len(f[0]) for f in frags]).astype(np.uint64)
    o2 = np.cumsum([0] + [len(f[1]) for f in frags]).astype(np.uint64)
    h1 = _hits([r for f in frags for r in f[0]])
    h2 = _hits([r for f in frags for r in f[1]])
    return h1, o1, np.array([f[2] for f in frags], dtype=np.uint32), h2, o2, np.array([f[3] for f in frags], dtype=np.uint32)


def _k(j):
    return j % 4


def _sc(j):
    return -1.0 - 0.125 * (j % 37)


def _cluster(n1, n2, base, frag):
    """n1 x n2, every cell concordant: forward hits at base + x, reverse hits at base + 200 + y (outer 300 + y - x)"""
    return ([(base + x, frag, 0, _k(x), _sc(x)) for x in range(n1)], [(base + 200 + y, frag, 1, _k(y + 1), _sc(y + 5)) for y in range(n2)], 100, 100)


def _line(flags, base, frag, transposed):
    """1 x len(flags) (transposed: len(flags) x 1): cell c is concordant iff flags[c]; positions are distinct"""
    one = [(base, frag, 0, 1, -2.5)]
    many = [((base + 100 + c) if f else (base + 5000 + c), frag, 1, _k(c), _sc(c)) for c, f in enumerate(flags)]
    if not transposed:
        return (one, many, 100, 100)
    # mate 2 is the forward one: reverse hits of mate 1 at base + 100 + c
    return ([(p, fr, 1, k, s) for p, fr, _, k, s in many], one, 100, 100)


def _diagonal(n, base, frag, dead_row=None):
    """n x n, concordant on the diagonal only (one cell in n); dead_row: that row's hit lies in another fragment"""
    a = [(base + 1000 * x, frag if x != dead_row else frag + 1, 0, _k(x), _sc(x)) for x in range(n)]
    b = [(base + 1000 * y + 200, frag, 1, _k(y + 2), _sc(y + 3)) for y in range(n)]
    return (a, b, 100, 100)


def _base_fragments():
    F = []
    # empty lists on either side and on both; 1 x 1 concordant and not
    F.append(([], [], 100, 100))
    F.append(([(10, 0, 0, 0, -1.0)], [], 100, 100))
    F.append(([], [(10, 0, 1, 0, -1.0)], 100, 100))
    F.append(([(1000, 0, 0, 0, -1.0)], [(1200, 0, 1, 2, -3.0)], 100, 100))
    F.append(([(1000, 0, 0, 0, -1.0)], [(1200, 0, 0, 0, -1.0)], 100, 100))       # same strand twice
    # outer distance exactly at the lower bound, one below, exactly at the upper bound, one above (bounds 150..420)
    for p2 in (1050, 1049, 1320, 1321):
        F.append(([(1000, 0, 0, 0, -1.0)], [(p2, 0, 1, 0, -1.0)], 100, 100))
    # containment (f.pos + len_f > r.pos + len_r), dovetail (the reverse mate starts in front), different fragments
    F.append(([(1000, 0, 0, 0, -1.0)], [(1010, 0, 1, 0, -1.0)], 200, 160))
    F.append(([(1000, 0, 0, 0, -1.0)], [(900, 0, 1, 0, -1.0)], 100, 300))
    F.append(([(1000, 0, 0, 0, -1.0)], [(1200, 1, 1, 0, -1.0)], 100, 100))
    # mate 2 forward, two placements
    F.append(([(2300, 2, 1, 2, -2.0), (7300, 2, 1, 3, -40.0)], [(2100, 2, 0, 0, -0.5), (7100, 2, 0, 1, -30.0)], 80, 120))
    # products of exactly the lane budget and one past it
    F.append(_cluster(4, 8, 20_000, 1))
    F.append(_cluster(3, 11, 30_000, 1))
    # 1 x 200 and 200 x 1: concordant cells in the first and the last lane of a 64-cell turn and on both sides of a turn
    # boundary (0, 63, 64), a turn of 64 concordant cells (128..191), a turn of none (192..199)
    flags = [c in (0, 63, 64, 100) or 128 <= c < 192 for c in range(200)]
    F.append(_line(flags, 40_000, 2, False))
    F.append(_line(flags, 60_000, 2, True))
    # 70 x 70 dense (every cell), 70 x 70 on the diagonal with one row entirely discordant, 20 x 20 sparse (1 cell in 20)
    F.append(_cluster(70, 70, 80_000, 3))
    F.append(_diagonal(70, 1_000_000, 4, dead_row=5))
    F.append(_diagonal(20, 2_000_000, 5))
    # 3 x 50: the step of 64 cells crosses a row (n2 < 64); the middle row is entirely discordant, the others mixed
    a = [(90_000, 6, 0, 1, -1.5), (90_001, 7, 0, 2, -2.5), (90_002, 6, 0, 3, -3.5)]
    b = [((90_200 + y) if y % 3 else (95_000 + y), 6, 1, _k(y), _sc(y)) for y in range(50)]
    F.append((a, b, 100, 100))
    return F


def _fragments(n):
    base = _base_fragments()
    return [base[i % len(base)] for i in range(n)]


_WANT = {}


def _want(n, fileid=0):
    """lists of n fragments and the checker's answer (computed once per n, shared and never changed)"""
    if (n, fileid) not in _WANT:
        L = _lists(_fragments(n))
        recs, off = pac.enumerate_pairs(*L, MIN_INS, MAX_INS, fileid)
        for a in L + (recs, off):
            a.setflags(write=False)
        _WANT[(n, fileid)] = (L, recs, off)
    return _WANT[(n, fileid)]


@pytest.fixture(scope="module")
def matchers():
    ms = {s: PairMatcher(_opts(32, 3, s, 2)) for s in (0, 1)}
    yield ms
    for m in ms.values():
        m.close()


def test_the_base_fragments_cover_what_they_claim():
    L, recs, off = _want(len(_base_fragments()))
    cnt = (off[1:] - off[:-1]).astype(np.int64).tolist()
    prod = pac.products(L[1], L[4]).tolist()
    assert cnt[:13] == [0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 2], cnt[:13]
    assert prod[13:15] == [32, 33] and cnt[13:15] == [32, 33]
    assert prod[15:17] == [200, 200] and cnt[15:17] == [68, 68]
    assert cnt[17:20] == [4900, 69, 20] and prod[19] == 400
    assert prod[20] == 150 and cnt[20] == 2 * 33
    np.testing.assert_array_equal(recs["outer"][off[5]:off[6]], [150])
    np.testing.assert_array_equal(recs["outer"][off[7]:off[8]], [420])
    assert (recs["inverted1"][off[12]:off[13]] == 1).all() and (recs["inverted1"][off[16]:off[17]] == 1).all()


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("n", [0, 1, 65, 300])
def test_pair_all_hits_against_the_checker(matchers, scores, n):
    m = matchers[scores]
    L, want, woff = _want(n)
    m.pair_all_stats(reset=True)
    got, off = m.pair_all_hits(*L, MIN_INS, MAX_INS, cap=max(1, want.shape[0]))
    np.testing.assert_array_equal(off, woff)
    pac.assert_pair_hits_equal(got, want, "n = %d" % n)
    st = m.pair_all_stats()
    exp = pac.expected_stats(L[1], L[4], want)
    assert st["fragments"] == n and {k: st[k] for k in exp} == exp, (st, exp)
    assert (st["launches"] > 0 or n == 0) and st["kernel_ms"] >= 0.0


def test_pair_all_hits_one_dense_fragment_alone(matchers):
    """n_pairs = 1 with a wave fragment (the single fragment of n = 1 above is an empty one)"""
    L = _lists([_cluster(70, 70, 80_000, 3)])
    want, woff = pac.enumerate_pairs(*L, MIN_INS, MAX_INS, 7)
    got, off = matchers[1].pair_all_hits(*L, MIN_INS, MAX_INS, fileid=7)
    assert want.shape[0] == 4900 and (want["fileid"] == 7).all()
    np.testing.assert_array_equal(off, woff)
    pac.assert_pair_hits_equal(got, want)


@pytest.mark.parametrize("scores", [1, 0])
def test_pair_all_hits_device_lists_and_null_offsets(matchers, scores):
    import torch
    m = matchers[scores]
    L, want, woff = _want(65)
    as_dev = {16: lambda x: x.view(np.int32).reshape(-1, 4), 8: lambda x: x.view(np.int64), 4: lambda x: x.view(np.int32)}
    dev = [torch.from_numpy(as_dev[x.dtype.itemsize](x).copy()).cuda() for x in L]
    out = torch.zeros(want.shape[0] * 32, dtype=torch.uint8, device="cuda")
    poff = torch.zeros(66, dtype=torch.int64, device="cuda")
    n_out, _ = m.pair_all_hits(*dev, MIN_INS, MAX_INS, out=out, pair_offsets=poff)
    assert n_out == want.shape[0]
    np.testing.assert_array_equal(poff.cpu().numpy().view(np.uint64), woff)
    pac.assert_pair_hits_equal(out.cpu().numpy().view(rlib.PAIR_HIT_DTYPE), want, "device lists")
    # pair_offsets NULL, host and device
    pp = PairMatcher._pair_params(MIN_INS, MAX_INS)
    nout = C.c_uint64(0)
    got = np.zeros(want.shape[0], dtype=rlib.PAIR_HIT_DTYPE)
    rc = m._L.real_hip_pair_all_hits(m._h, C.byref(pp), *[x.ctypes.data for x in L], 65, 0, 0, got.ctypes.data, got.shape[0], C.byref(nout), None)
    assert rc == 0 and nout.value == want.shape[0]
    pac.assert_pair_hits_equal(got, want, "null offsets, host")
    out.zero_()
    torch.cuda.synchronize()
    rc = m._L.real_hip_pair_all_hits(m._h, C.byref(pp), *[x.data_ptr() for x in dev], 65, 0, 1, out.data_ptr(), want.shape[0], C.byref(nout), None)
    assert rc == 0 and nout.value == want.shape[0]
    pac.assert_pair_hits_equal(out.cpu().numpy().view(rlib.PAIR_HIT_DTYPE), want, "null offsets, device")


def test_pair_all_hits_follows_the_input_order(matchers):
    """shuffled lists: the output is the row-major walk of the SHUFFLED lists (nothing is sorted), and as a set it is the
    same pairs"""
    rng = np.random.default_rng(9)
    F = _fragments(len(_base_fragments()))
    G = [([a[j] for j in rng.permutation(len(a))], [b[j] for j in rng.permutation(len(b))], la, lb) for a, b, la, lb in F]
    L = _lists(G)
    want, woff = pac.enumerate_pairs(*L, MIN_INS, MAX_INS)
    got, off = matchers[1].pair_all_hits(*L, MIN_INS, MAX_INS)
    np.testing.assert_array_equal(off, woff)
    pac.assert_pair_hits_equal(got, want, "shuffled")
    _, straight, soff = _want(len(F))
    np.testing.assert_array_equal(off, soff)
    assert not np.array_equal(got, straight)
    key = lambda r: np.sort(r, order=["pair", "pos1", "pos2", "inverted1"])
    pac.assert_pair_hits_equal(key(got), key(straight), "the same set")


def test_pair_all_hits_overflow(matchers):
    m = matchers[1]
    L, want, woff = _want(65)
    need = want.shape[0]
    pp = PairMatcher._pair_params(MIN_INS, MAX_INS)
    ptr = [x.ctypes.data for x in L]
    nout = C.c_uint64(0)
    out = np.zeros(need, dtype=rlib.PAIR_HIT_DTYPE)
    out["pair"] = 0xdeadbeef
    poff = np.zeros(66, dtype=np.uint64)
    rc = m._L.real_hip_pair_all_hits(m._h, C.byref(pp), *ptr, 65, 0, 0, out.ctypes.data, need - 1, C.byref(nout), poff.ctypes.data)
    assert rc == rlib.REAL_HIP_E_OVERFLOW and nout.value == need
    assert (out["pair"] == 0xdeadbeef).all() and not out["pos1"].any(), "out must stay untouched"
    rc = m._L.real_hip_pair_all_hits(m._h, C.byref(pp), *ptr, 65, 0, 0, out.ctypes.data, need, C.byref(nout), poff.ctypes.data)
    assert rc == 0 and nout.value == need
    pac.assert_pair_hits_equal(out, want, "cap == needed")
    # cap == 0 with zero pairs (the first three fragments are empty products)
    L3 = _lists(_base_fragments()[:3])
    rc = m._L.real_hip_pair_all_hits(m._h, C.byref(pp), *[x.ctypes.data for x in L3], 3, 0, 0, None, 0, C.byref(nout), poff.ctypes.data)
    assert rc == 0 and nout.value == 0 and not poff[:4].any()
    # the wrapper retries with the size the library reports
    got, off = m.pair_all_hits(*L, MIN_INS, MAX_INS, cap=5)
    pac.assert_pair_hits_equal(got, want, "retry")


@pytest.mark.parametrize("scores", [1, 0])
def test_pair_all_hits_agrees_with_the_join(matchers, scores):
    """the shipped join on the same lists: its records' best location and second value follow from the enumerated list"""
    m = matchers[scores]
    L, _, _ = _want(len(_base_fragments()))
    got, off = m.pair_all_hits(*L, MIN_INS, MAX_INS)
    rec = m.pair_hits(*L, MIN_INS, MAX_INS)
    pac.assert_consistent_with_records(got, off, rec, bool(scores), "join")
    assert (rec["state"] != rlib.PAIR_NOMATCH).sum() == ((off[1:] - off[:-1]) > 0).sum()


def test_pair_all_errors_are_loud(matchers):
    m = matchers[1]
    L, want, _ = _want(65)
    ptr = [x.ctypes.data for x in L]
    out = np.zeros(want.shape[0], dtype=rlib.PAIR_HIT_DTYPE)
    nout = C.c_uint64(0)

    def call(pp, o=out.ctypes.data, cap=out.shape[0], no=C.byref(nout)):
        return m._L.real_hip_pair_all_hits(m._h, C.byref(pp) if pp is not None else None, *ptr, 65, 0, 0, o, cap, no, None)
    pp = PairMatcher._pair_params(MIN_INS, MAX_INS)
    pp.struct_size = 12
    assert call(pp) == rlib.REAL_HIP_E_INVALID
    assert call(PairMatcher._pair_params(421, 420)) == rlib.REAL_HIP_E_INVALID
    assert call(PairMatcher._pair_params(MIN_INS, MAX_INS, 1)) == rlib.REAL_HIP_E_UNSUPPORTED
    assert call(PairMatcher._pair_params(MIN_INS, MAX_INS), o=None) == rlib.REAL_HIP_E_INVALID        # null out with cap > 0
    assert call(PairMatcher._pair_params(MIN_INS, MAX_INS), no=None) == rlib.REAL_HIP_E_INVALID
    assert call(None) == rlib.REAL_HIP_E_INVALID
    with pytest.raises(rlib.RealHipError) as e:
        m.pair_all_hits(*L, MIN_INS, MAX_INS, orientation=2)
    assert e.value.status == rlib.REAL_HIP_E_UNSUPPORTED
    with pytest.raises(rlib.RealHipError) as e:
        m.match_pairs_all((np.zeros(100, np.uint8), None, np.array([0, 100], np.uint64)),
                          (np.zeros(100, np.uint8), None, np.array([0, 100], np.uint64)), MIN_INS, MAX_INS)
    assert e.value.status == rlib.REAL_HIP_E_STATE                                                   # no text / index
    assert not out.view(np.uint8).any()
    # the context still works
    got, _ = m.pair_all_hits(*L, MIN_INS, MAX_INS)
    pac.assert_pair_hits_equal(got, want, "after the errors")


# ---- the whole path: matchAll of both mates on the device, then the enumeration ---------------------------------------
# scores, totalkmax, filter_level, table_kind, prefix_bits, seedl, ragged, (patl1, patl2), on_device
CASES = [(1, 3, 2, 0, 0, 32, False, (100, 100), 0),
         (0, 3, 2, 3, 13, 16, True, (100, 80), 1),
         (1, 3, 2, 3, 13, 16, True, (100, 100), 0),
         (0, 3, 2, 0, 0, 32, False, (100, 80), 1)]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", ["iid", "families"])
def test_match_pairs_all_against_the_checker(ora, kind, case):
    scores, tk, fl, tkind, pb, seedl, ragged, patl, on_device = case
    g, b1, b2 = pw.pair_workload(kind, ragged, patl, n=1500)
    (_, h1, o1, h2, o2), _ = pw.oracle_pairs(ora, g, b1, b2, seedl, tk, scores, fl)
    l1, l2 = pw.lens_of(b1), pw.lens_of(b2)
    want, woff = pac.enumerate_pairs(h1, o1, l1, h2, o2, l2, pw.MIN_INS, pw.MAX_INS, 0)
    exp = pac.expected_stats(o1, o2, want)
    per = (woff[1:] - woff[:-1]).astype(np.int64)
    print(kind, case, exp, "fragments with >= 2 pairs:", int((per >= 2).sum()))
    assert want.shape[0] > 500
    if kind == "families":
        assert (per >= 2).sum() >= 20 and exp["handed_over"] > 0, (int((per >= 2).sum()), exp)
    m = PairMatcher(_opts(seedl, tk, scores, fl), prefix_bits=pb, table_kind=tkind)
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    n = b1.n_reads
    if not on_device:
        got, off = m.match_pairs_all(b1, b2, pw.MIN_INS, pw.MAX_INS, cap=7)           # too small: overflow and retry inside
        np.testing.assert_array_equal(off, woff)
        pac.assert_pair_hits_equal(got, want, "%s %r" % (kind, case))
        m.pair_all_stats(reset=True)
        got, off = m.match_pairs_all(b1, b2, pw.MIN_INS, pw.MAX_INS, cap=want.shape[0])
    else:
        import torch
        dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)]
        small = torch.zeros(7 * 32, dtype=torch.uint8, device="cuda")
        poff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        with pytest.raises(rlib.RealHipError) as e:                                    # too small: the size needed is reported
            m.match_pairs_all(dev[0], dev[1], pw.MIN_INS, pw.MAX_INS, out=small, pair_offsets=poff)
        assert e.value.status == rlib.REAL_HIP_E_OVERFLOW and e.value.needed == want.shape[0] and not small.any()
        m.pair_all_stats(reset=True)
        out = torch.zeros(e.value.needed * 32, dtype=torch.uint8, device="cuda")
        n_out, _ = m.match_pairs_all(dev[0], dev[1], pw.MIN_INS, pw.MAX_INS, out=out, pair_offsets=poff)
        assert n_out == want.shape[0]
        got, off = out.cpu().numpy().view(rlib.PAIR_HIT_DTYPE), poff.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(off, woff)
    pac.assert_pair_hits_equal(got, want, "%s %r" % (kind, case))
    st = m.pair_all_stats()
    assert st["fragments"] == n and {k: st[k] for k in exp} == exp, (st, exp)
    m.close()
