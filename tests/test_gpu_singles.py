"""Single placements of a mate on the device (real_hip_single_hits / real_hip_match_pairs_singles) against the brute-force
checker of singles_checker.py, which works from hand-made lists or the oracle's match_all lists and never calls the code
under test.  Every field is compared, the floats bit for bit."""
import ctypes as C

import numpy as np
import pytest

import pairs_checker as pc
import pairs_workloads as pw
import singles_checker as sc
import singles_workloads as sw
from real_amd import lib as rlib
from real_amd.matcher import PairMatcher, RealOptions, new_pair_info, new_single_info

pytestmark = pytest.mark.gpu
LEN, FM = 100, 3 / 70.0            # read length of the hand-made reads; filter_mult of -e 3 -filter_level 2


def _opts(seedl, totalkmax, scores, filter_level):
    return RealOptions(seedl=seedl, seedkmax=2, totalkmax=totalkmax, scores=bool(scores), filter_level=filter_level).normalise()


@pytest.fixture(scope="module")
def matchers():
    import torch
    torch.zeros(1, device="cuda")      # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    ms = {s: PairMatcher(_opts(32, 3, s, 2)) for s in (0, 1)}
    assert ms[1].opts.filter_mult == FM
    yield ms
    for m in ms.values():
        m.close()


# ---- hand-made lists ------------------------------------------------------------------------------------------------------
def _hits(rows):
    """rows of (pos, frag, inverted, k, score)"""
    h = np.zeros(len(rows), dtype=rlib.HIT_DTYPE)
    for j, (pos, frag, inv, k, score) in enumerate(rows):
        h[j] = (0, pos, score, frag, k, inv)
    return h


def _row(scores, pos, frag, inv, k, score):
    """with scores off the value is -k and a hit's score is 1.0f"""
    return (pos, frag, inv, k, score if scores else 1.0)


def _long_list(scores, n, best_at, tie_at=None, base=10_000):
    """n hits at distinct positions, all far below the one at index best_at (and, for a tie, the one at tie_at: the same
    value at a LARGER location)"""
    rows = [_row(scores, base + 10 * j, 2, j & 1, 3, -40.0 - (j % 7)) for j in range(n)]
    p, f, inv, _, _ = rows[best_at]
    rows[best_at] = _row(scores, p, f, inv, 1, -2.5)
    if tie_at is not None:
        p, f, inv, _, _ = rows[tie_at]
        assert tie_at > best_at
        rows[tie_at] = _row(scores, p, f, inv, 1, -2.5)
    return rows


def _hand_reads(scores):
    """[(rows, what the checker must say: state, pos, inverted) ...]"""
    eps = sc.eps_of(True, FM, LEN)
    at = np.float32(np.float64(-1.0) - np.float64(eps))
    assert np.float64(at) == np.float64(-1.0) - np.float64(eps), "best - eps is a float: the boundary can be hit exactly"
    below = np.nextafter(at, np.float32(-np.inf))
    R = []
    R.append(([], (sc.NOMATCH, 0, 0)))                                                                       # an empty list
    R.append(([_row(scores, 777, 1, 1, 2, -3.25)], (sc.UNIQUE, 777, 1)))                                        # one hit
    R.append(([_row(scores, 5000, 1, 0, 1, -3.0), _row(scores, 900, 1, 0, 1, -3.0)], (sc.NONUNIQUE, 900, 0)))   # equal values: the smaller location
    R.append(([_row(scores, 4000, 0, 1, 0, -1.5), _row(scores, 4000, 0, 0, 0, -1.5)], (sc.NONUNIQUE, 4000, 0)))  # one position, both strands
    if scores:   # second exactly at best - eps, and one float step below
        R.append(([_row(1, 100, 0, 0, 0, -1.0), _row(1, 9000, 0, 0, 3, float(at))], (sc.NONUNIQUE, 100, 0)))
        R.append(([_row(1, 100, 0, 0, 0, -1.0), _row(1, 9000, 0, 0, 3, float(below))], (sc.UNIQUE, 100, 0)))
    else:        # eps = 0: second exactly at best (the same k), and one step below (one mismatch more)
        R.append(([_row(0, 100, 0, 0, 0, 0), _row(0, 9000, 0, 0, 0, 0)], (sc.NONUNIQUE, 100, 0)))
        R.append(([_row(0, 100, 0, 0, 0, 0), _row(0, 9000, 0, 0, 1, 0)], (sc.UNIQUE, 100, 0)))
    R.append((_long_list(scores, 32, 31), (sc.UNIQUE, 10_310, 1)))                                              # the two sides of a lane's budget
    R.append((_long_list(scores, 33, 32), (sc.UNIQUE, 10_320, 0)))
    R.append((_long_list(scores, 64, 63), (sc.UNIQUE, 10_630, 1)))                                              # the last lane of the only turn
    R.append((_long_list(scores, 65, 64), (sc.UNIQUE, 10_640, 0)))                                              # the first lane of the second turn
    R.append((_long_list(scores, 65, 0), (sc.UNIQUE, 10_000, 0)))                                               # the first lane of the first turn
    R.append((_long_list(scores, 200, 127), (sc.UNIQUE, 11_270, 1)))                                            # the last lane of the second turn
    R.append((_long_list(scores, 200, 128), (sc.UNIQUE, 11_280, 0)))                                            # the first lane of the third turn
    R.append((_long_list(scores, 200, 10, tie_at=74), (sc.NONUNIQUE, 10_100, 0)))                               # a tie across two turns, one lane
    R.append((_long_list(scores, 200, 63, tie_at=192), (sc.NONUNIQUE, 10_630, 1)))                              # a tie across the first and the last turn
    return R


def _lists(reads):
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    return _hits([x for r in reads for x in r]), off, np.full(len(reads), LEN, dtype=np.uint32)


def _reads(scores, n):
    base = [r for r, _ in _hand_reads(scores)]
    return [base[i % len(base)] for i in range(n)]


@pytest.mark.parametrize("scores", [1, 0])
def test_single_hits_on_hand_made_lists(matchers, scores):
    m = matchers[scores]
    hand = _hand_reads(scores)
    L = _lists([r for r, _ in hand])
    want = sc.check_singles([(0, L[0], L[1])], L[2], scores, FM)
    for i, (_, (state, pos, inv)) in enumerate(hand):      # the checker says what the cases were built for
        assert (int(sc.state_of(want["tag"][i])), int(want["pos"][i]), int(sc.inverted_of(want["tag"][i]))) == (state, pos, inv), (i, want[i])
    assert want[0].tobytes() == sc.empty_record().tobytes() and np.isneginf(want["second"][1])
    if not scores:
        assert want["second"][4].tobytes() == np.float32(-0.0).tobytes() and want["score"][4] == 1.0    # -(float)k of k = 0
    m.single_stats(reset=True)
    got = m.single_hits(*L)
    sc.assert_singles_equal(got, want, "host lists")
    st = m.single_stats()
    longer = sum(len(r) > 32 for r, _ in hand)
    assert longer == 8 and (st["reads"], st["hits"], st["handed_over"], st["launches"]) == (len(hand), int(L[1][-1]), longer, 2), st


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("n", [0, 1, 65, 300])
def test_single_hits_read_counts_host_and_device(matchers, scores, n):
    import torch
    m = matchers[scores]
    reads = _reads(scores, n)
    if n == 1:
        reads = [_long_list(scores, 200, 128)]         # one read, and a wave's
    L = _lists(reads)
    want = sc.check_singles([(0, L[0], L[1])], L[2], scores, FM)
    m.single_stats(reset=True)
    sc.assert_singles_equal(m.single_hits(*L), want, "host lists")
    st = m.single_stats()
    assert (st["reads"], st["hits"], st["handed_over"]) == (n, int(L[1][-1]), sum(len(r) > 32 for r in reads)), st
    as_dev = {16: lambda x: x.view(np.int32).reshape(-1, 4), 8: lambda x: x.view(np.int64), 4: lambda x: x.view(np.int32)}
    dev = [torch.from_numpy(as_dev[x.dtype.itemsize](x).copy()).cuda() for x in L]
    rec = torch.full((max(n, 1) * 16,), 0xAB, dtype=torch.uint8, device="cuda")       # fresh: output only, whatever it held
    m.single_hits(*dev, singles=rec, fresh=True)
    if n:
        sc.assert_singles_equal(rec.cpu().numpy().view(rlib.SINGLE_DTYPE)[:n], want, "device lists")
    else:
        assert (rec.cpu().numpy() == 0xAB).all()


@pytest.mark.parametrize("scores", [1, 0])
def test_single_hits_order_and_folds(matchers, scores):
    m = matchers[scores]
    reads = _reads(scores, 65)
    L = _lists(reads)
    want = sc.check_singles([(0, L[0], L[1])], L[2], scores, FM)
    rng = np.random.default_rng(4)
    for what in ("reversed", "shuffled"):
        G = [r[::-1] if what == "reversed" else [r[j] for j in rng.permutation(len(r))] for r in reads]
        sc.assert_singles_equal(m.single_hits(*_lists(G)), want, what)
    # the same list again with fresh = 0 changes nothing: a location counts once
    rec = m.single_hits(*L)
    again = m.single_hits(*L, singles=rec.copy())
    sc.assert_singles_equal(again, want, "the same file folded twice")
    # the same lists as file 1: every location exists twice, NonUnique through the file id alone, file 0 reported
    both = m.single_hits(*L, fileid=1, singles=rec.copy())
    want2 = sc.check_singles([(0, L[0], L[1]), (1, L[0], L[1])], L[2], scores, FM)
    sc.assert_singles_equal(both, want2, "the same lists as two files")
    had = sc.state_of(want["tag"]) != sc.NOMATCH
    assert had.any() and (sc.state_of(both["tag"])[had] == sc.NONUNIQUE).all() and (both["fileid"][had] == 0).all()
    # two different files in both orders, and the lists of one file in two blocks
    other = [reads[(i * 7 + 3) % len(reads)] for i in range(len(reads))]
    other = [[(p + 5, f, inv, k, s) for p, f, inv, k, s in r[:40]] for r in other]
    L2 = _lists(other)
    ab = m.single_hits(*L2, fileid=1, singles=m.single_hits(*L, fileid=0))
    ba = m.single_hits(*L, fileid=0, singles=m.single_hits(*L2, fileid=1))
    want3 = sc.check_singles([(0, L[0], L[1]), (1, L2[0], L2[1])], L[2], scores, FM)
    sc.assert_singles_equal(ab, want3, "files 0, 1")
    sc.assert_singles_equal(ba, want3, "files 1, 0")
    halves = [_lists([r[:len(r) // 2] for r in reads]), _lists([r[len(r) // 2:] for r in reads])]
    blocks = m.single_hits(*halves[1], singles=m.single_hits(*halves[0]))
    sc.assert_singles_equal(blocks, want, "one file in two blocks")
    # an empty input record is empty whatever its other fields hold
    junk = new_single_info(len(reads))
    junk["score"], junk["second"], junk["pos"], junk["frag"], junk["fileid"], junk["tag"] = 7.0, 5.0, 123, 4, 9, 0x1F
    sc.assert_singles_equal(m.single_hits(*L, singles=junk), want, "empty input records")


def test_single_errors_are_loud(matchers):
    import torch
    m = matchers[1]
    L = _lists(_reads(1, 20))
    h, off, lens = L
    rec = new_single_info(20)
    call = m._L.real_hip_single_hits
    ok = (h.ctypes.data, off.ctypes.data, lens.ctypes.data, 20, 0, 0, 1, rec.ctypes.data)
    assert call(m._h, *ok) == rlib.REAL_HIP_OK
    bad = off.copy()
    bad[0] = 1
    assert call(m._h, h.ctypes.data, bad.ctypes.data, *ok[2:]) == rlib.REAL_HIP_E_INVALID              # offsets not starting at 0
    dev_bad = torch.from_numpy(bad.view(np.int64).copy()).cuda()
    dev_h = torch.from_numpy(h.view(np.int32).reshape(-1, 4).copy()).cuda()
    dev_len = torch.from_numpy(lens.view(np.int32).copy()).cuda()
    dev_rec = torch.zeros(20 * 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert call(m._h, dev_h.data_ptr(), dev_bad.data_ptr(), dev_len.data_ptr(), 20, 0, 1, 1, dev_rec.data_ptr()) == rlib.REAL_HIP_E_INVALID
    bad = off.copy()
    bad[5] = bad[6] + 1
    assert call(m._h, h.ctypes.data, bad.ctypes.data, *ok[2:]) == rlib.REAL_HIP_E_INVALID              # offsets running backwards
    assert call(m._h, None, *ok[1:]) == rlib.REAL_HIP_E_INVALID                                        # a null list with hits
    assert call(m._h, *ok[:4], 256, 0, 1, rec.ctypes.data) == rlib.REAL_HIP_E_INVALID                   # fileid 256
    assert call(m._h, *ok[:7], None) == rlib.REAL_HIP_E_INVALID                                        # null records
    assert call(m._h, ok[0], None, *ok[2:]) == rlib.REAL_HIP_E_INVALID and call(m._h, ok[0], ok[1], None, *ok[3:]) == rlib.REAL_HIP_E_INVALID
    assert call(m._h, None, None, None, 0, 0, 0, 1, None) == rlib.REAL_HIP_OK                          # no reads: nothing to do
    st = rlib.RealHipSingleStats()
    st.struct_size = C.sizeof(rlib.RealHipSingleStats) - 8
    assert m._L.real_hip_single_stats_get(m._h, C.byref(st), 0) == rlib.REAL_HIP_E_INVALID
    # the context still works
    sc.assert_singles_equal(m.single_hits(*L), sc.check_singles([(0, h, off)], lens, 1, FM), "after the errors")


# ---- the whole path ---------------------------------------------------------------------------------------------------------
def _matcher(w, case):
    scores, tk, fl, seedl, _, _, tkind, pb = case
    m = PairMatcher(_opts(seedl, tk, scores, fl), prefix_bits=pb, table_kind=tkind)
    m.set_text_symbols(0, w["g"].sym, w["g"].frag_start)
    m.build_index_block()
    assert m.table_kind == {0: rlib.LAYOUT_STARTS, 3: rlib.LAYOUT_ROWS}[tkind], m.table_kind
    return m


@pytest.mark.parametrize("case", sw.CASES)
@pytest.mark.parametrize("kind", sw.KINDS)
def test_match_pairs_singles_against_the_checkers(ora, kind, case):
    import torch
    w = sw.workload(ora, kind, case)
    print(kind, case, w["classes"], w["longer_than_32"])
    sw.assert_coverage(w, kind)
    b1, b2, n = w["b1"], w["b2"], w["b1"].n_reads
    m = _matcher(w, case)
    plain = m.match_pairs(b1, b2, pw.MIN_INS, pw.MAX_INS)
    m.single_stats(reset=True)
    pairs, s1, s2 = m.match_pairs_singles(b1, b2, pw.MIN_INS, pw.MAX_INS)
    st = m.single_stats()
    pc.assert_records_equal(pairs, w["pairs"], "pairs %s %r" % (kind, case))
    assert pairs.tobytes() == plain.tobytes(), "pairs differ from real_hip_match_pairs"
    sc.assert_singles_equal(s1, w["s1"], "mate 1 %s %r" % (kind, case))
    sc.assert_singles_equal(s2, w["s2"], "mate 2 %s %r" % (kind, case))
    assert (st["reads"], st["hits"], st["handed_over"], st["launches"]) == (2 * n, w["hits"], w["longer_than_32"], 2), (st, w["hits"], w["longer_than_32"])
    if kind == "families":
        assert st["handed_over"] > 0
    # the same file again into the records (fresh = 0): nothing changes
    p2, t1, t2 = m.match_pairs_singles(b1, b2, pw.MIN_INS, pw.MAX_INS, pairs=pairs.copy(), singles1=s1.copy(), singles2=s2.copy())
    sc.assert_singles_equal(t1, w["s1"], "mate 1 folded twice")
    sc.assert_singles_equal(t2, w["s2"], "mate 2 folded twice")
    # batches and outputs on the device
    dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)]
    dp = torch.full((n * 40,), 0xCD, dtype=torch.uint8, device="cuda")
    d1 = torch.full((n * 16,), 0xCD, dtype=torch.uint8, device="cuda")
    d2 = torch.full((n * 16,), 0xCD, dtype=torch.uint8, device="cuda")
    m.match_pairs_singles(dev[0], dev[1], pw.MIN_INS, pw.MAX_INS, pairs=dp, singles1=d1, singles2=d2, fresh=True)
    assert dp.cpu().numpy().tobytes() == plain.tobytes()
    sc.assert_singles_equal(d1.cpu().numpy().view(rlib.SINGLE_DTYPE), w["s1"], "mate 1, device outputs")
    sc.assert_singles_equal(d2.cpu().numpy().view(rlib.SINGLE_DTYPE), w["s2"], "mate 2, device outputs")
    m.close()


def test_match_pairs_singles_with_the_mate_search(ora):
    """with sp the pairs are real_hip_match_pairs_search's, and the singles stay folds of seed hits"""
    kind, case = "families", sw.CASES[0]
    w = sw.workload(ora, kind, case)
    b1, b2 = w["b1"], w["b2"]
    m = _matcher(w, case)
    searched = m.match_pairs(b1, b2, pw.MIN_INS, pw.MAX_INS, mate_search=True)
    pairs, s1, s2 = m.match_pairs_singles(b1, b2, pw.MIN_INS, pw.MAX_INS, mate_search=True)
    assert pairs.tobytes() == searched.tobytes()
    print("fragments the search changes:", int((searched["state"] != w["pairs"]["state"]).sum()))
    sc.assert_singles_equal(s1, w["s1"], "mate 1 with the search")
    sc.assert_singles_equal(s2, w["s2"], "mate 2 with the search")
    # loud: null singles, a wrong search struct
    bb1, bb2 = m._mate_batch(b1), m._mate_batch(b2)
    pp = PairMatcher._pair_params(pw.MIN_INS, pw.MAX_INS)
    rec, x1 = new_pair_info(b1.n_reads), new_single_info(b1.n_reads)
    call = m._L.real_hip_match_pairs_singles
    assert call(m._h, C.byref(bb1), C.byref(bb2), C.byref(pp), None, rec.ctypes.data, x1.ctypes.data, None) == rlib.REAL_HIP_E_INVALID
    assert call(m._h, C.byref(bb1), C.byref(bb2), C.byref(pp), None, None, x1.ctypes.data, x1.ctypes.data) == rlib.REAL_HIP_E_INVALID
    sp = PairMatcher._search_params(0)
    sp.struct_size = 8
    assert call(m._h, C.byref(bb1), C.byref(bb2), C.byref(pp), C.byref(sp), rec.ctypes.data, x1.ctypes.data, x1.ctypes.data) == rlib.REAL_HIP_E_INVALID
    m.close()
