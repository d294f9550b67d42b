"""Mapping quality on the device (real_hip_mapq_hits / _pair_hits / real_hip_match_mapq / _pairs_mapq / real_hip_mapq / _pairs)
against the brute-force checker of mapq_checker.py, which works from hand-made lists or the oracle's match_all lists in Python
integers and never calls the code under test.  Accumulators and qualities are compared byte for byte."""
import ctypes as C

import numpy as np
import pytest

import mapq_checker as mq
import mapq_workloads as mw
import mate_search_workloads as msw
import pairs_workloads as pw
from real_amd import lib as rlib
from real_amd.matcher import PairMatcher, RealOptions, new_mapq_acc, new_pair_info, new_single_info, unpack_info

pytestmark = pytest.mark.gpu
LEN = 100
RISES = [0, 1, 7, 8, 9, 16, 24, 31, 32, 40]      # of the window's top: inside a count word, across each of the four, and out of it


def _opts(seedl, totalkmax, scores, filter_level):
    return RealOptions(seedl=seedl, seedkmax=2, totalkmax=totalkmax, scores=bool(scores), filter_level=filter_level).normalise()


@pytest.fixture(scope="module")
def matchers():
    import torch
    torch.zeros(1, device="cuda")      # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    ms = {s: PairMatcher(_opts(32, 3, s, 2)) for s in (0, 1)}
    yield ms
    for m in ms.values():
        m.close()


def _dev(x):
    """a host array of the ABI as a device tensor of the same bytes"""
    import torch
    as_dev = {40: lambda a: a.view(np.int64).reshape(-1, 5), 16: lambda a: a.view(np.int32).reshape(-1, 4), 8: lambda a: a.view(np.int64),
              4: lambda a: a.view(np.int32), 1: lambda a: a}
    return torch.from_numpy(as_dev[x.dtype.itemsize](np.ascontiguousarray(x)).copy()).cuda()


def _same(got, want, what=""):
    got, want = np.asarray(got).view(np.uint8).reshape(-1), np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d bytes differ, the first in record %d" % (what, bad.size, bad[0] // 40)


# ---- hand-made lists ------------------------------------------------------------------------------------------------------
def _hits(rows):
    """rows of (pos, frag, inverted, k, score)"""
    h = np.zeros(len(rows), dtype=rlib.HIT_DTYPE)
    for j, (pos, frag, inv, k, score) in enumerate(rows):
        h[j] = (0, pos, score, frag, k, inv)
    return h


def _hit(j, level, k):
    """hit j of a list: with scores on its level is `level` (a score of level / 2 + 1 / 4 is exact), with scores off -12 k"""
    return (1000 + 10 * j, 1, j & 1, k, level / 2 + 0.25)


def _rising(n, start=-100):
    """n hits whose levels climb through RISES (the top rises by each of them when the hits come in this order), then repeat"""
    levels, top = [], start
    for j in range(n):
        top += RISES[j % len(RISES)]
        levels.append(top)
    return [_hit(j, lv, (3 * j) % 5) for j, lv in enumerate(levels)]


def _hand_reads():
    R = [[], [_hit(0, -1, 2)]]                                                          # empty; one hit at score -0.25
    for n in (32, 33, 64, 65):                                                          # both sides of a lane's budget, of a wave's turn
        R.append([_hit(j, 5 - (j % 9), j % 4) for j in range(n)])
    R.append([_hit(j, -7, 1) for j in range(300)])                                      # 300 equal: the count saturates at 255
    R.append([_hit(j, -7 - (j % 2) * 31, j % 2) for j in range(300)])                    # two saturated counts at the window's two ends
    R.append([_hit(j, 3 - 32 * (j % 2), 0 if j % 2 else 3) for j in range(40)])          # half of them one level outside the window
    R += [_rising(n) for n in (10, 20, 32, 33, 65, 300)]                                # the top rises across every count word, lane and wave
    R += [list(reversed(_rising(n))) for n in (20, 300)]                                # and never rises: the best first
    return R


def _lists(reads):
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    return _hits([x for r in reads for x in r]), off


def _reads(n):
    base = _hand_reads()
    return [base[i % len(base)] for i in range(n)]


@pytest.mark.parametrize("scores", [1, 0])
def test_mapq_hits_on_hand_made_lists(matchers, scores):
    m = matchers[scores]
    reads = _hand_reads()
    h, off = _lists(reads)
    want = mq.check_hits([(h, off)], len(reads), scores)
    assert want == mq.check_hits([(h, off)], len(reads), scores, count=mq.sorted_acc_of_levels)
    assert want[0] == mq.empty() and want[6]["cnt"][0] == 255 and want[6]["n"] == 300       # the checker says what the cases were built for
    if scores:
        assert want[1] == mq.acc_of_levels([-1]) and (want[7]["cnt"][0], want[7]["cnt"][31]) == (150, 150) and sum(want[8]["cnt"]) == 20
        assert want[14]["level"] == -100 + 30 * sum(RISES) and want[14] == want[16]
    else:
        assert want[1] == mq.acc_of_levels([-24]) and want[7]["cnt"][0] == want[7]["cnt"][12] == 150 and sum(want[8]["cnt"]) == 20
    m.mapq_stats(reset=True)
    got = m.mapq_hits(h, off)
    _same(got, mq.acc_records(want), "host lists")
    st = m.mapq_stats()
    longer = sum(len(r) > 32 for r in reads)
    assert longer >= 8 and (st["folded"], st["candidates"], st["handed_over"], st["launches"]) == (len(reads), int(off[-1]), longer, 2), st


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("n", [0, 1, 65, 300])
def test_mapq_hits_read_counts_host_and_device(matchers, scores, n):
    import torch
    m = matchers[scores]
    reads = _reads(n) if n != 1 else [_rising(300)]            # one read, and a wave's
    h, off = _lists(reads)
    want = mq.acc_records(mq.check_hits([(h, off)], n, scores))
    m.mapq_stats(reset=True)
    _same(m.mapq_hits(h, off), want, "host lists")
    st = m.mapq_stats()
    assert (st["folded"], st["candidates"], st["handed_over"]) == (n, int(off[-1]), sum(len(r) > 32 for r in reads)), st
    rec = torch.full((max(n, 1) * 40,), 0xAB, dtype=torch.uint8, device="cuda")       # fresh: output only, whatever it held
    m.mapq_hits(_dev(h) if len(h) else torch.zeros((1, 4), dtype=torch.int32, device="cuda"), _dev(off), acc=rec, fresh=True)
    if n:
        _same(rec.cpu().numpy(), want, "device lists")
    else:
        assert (rec.cpu().numpy() == 0xAB).all()


@pytest.mark.parametrize("scores", [1, 0])
def test_mapq_hits_order_and_folds(matchers, scores):
    m = matchers[scores]
    reads = _reads(65)
    h, off = _lists(reads)
    accs = mq.check_hits([(h, off)], 65, scores)
    want = mq.acc_records(accs)
    rng = np.random.default_rng(4)
    for what in ("reversed", "shuffled"):
        G = [r[::-1] if what == "reversed" else [r[j] for j in rng.permutation(len(r))] for r in reads]
        _same(m.mapq_hits(*_lists(G)), want, what)
    # one call against two calls on the halves of the lists, in both orders; and interleaved halves
    for split in (lambda r: (r[:len(r) // 2], r[len(r) // 2:]), lambda r: (r[::2], r[1::2])):
        halves = [_lists([split(r)[0] for r in reads]), _lists([split(r)[1] for r in reads])]
        _same(m.mapq_hits(*halves[1], acc=m.mapq_hits(*halves[0])), want, "two blocks")
        _same(m.mapq_hits(*halves[0], acc=m.mapq_hits(*halves[1])), want, "two blocks, the other order")
    # the same lists again with fresh = 0: every candidate twice (the fold counts, it does not look at locations)
    twice = mq.acc_records([mq.merge(a, a) for a in accs])
    _same(m.mapq_hits(h, off, acc=m.mapq_hits(h, off)), twice, "folded twice")
    # an input record with n = 0 is empty whatever its other fields hold
    junk = new_mapq_acc(65)
    junk["level"], junk["cnt"] = 77, 9
    _same(m.mapq_hits(h, off, acc=junk), want, "empty input records")
    # device records folded into (fresh = 0)
    dacc = _dev(want)
    m.mapq_hits(_dev(h), _dev(off), acc=dacc, fresh=False)
    _same(dacc.cpu().numpy(), twice, "device records folded into")


# ---- the concordant pairs of hand-made lists ---------------------------------------------------------------------------------
MIN_INS, MAX_INS = 150, 420


def _pair_fragments():
    """[(rows of mate 1, rows of mate 2)]: mate 1 forward at 1000 + 3 x, mate 2 reverse so that the outer distance is d"""
    def fwd(x, level, k):
        return (1000 + 3 * x, 2, 0, k, level / 2 + 0.25)

    def rev(outer, level, k, at=1000):
        return (at + outer - LEN, 2, 1, k, level / 2 + 0.25)
    F = [([], []), ([fwd(0, -3, 1)], []), ([], [rev(300, -3, 1)])]
    F.append(([fwd(0, -3, 1)], [rev(300, -5, 2)]))                                                   # one pair
    F.append(([fwd(0, -3, 1), (5000, 2, 0, 0, 0.25)], [(1200, 2, 0, 1, -1.25), (5300, 3, 1, 1, -1.25)]))   # both forward; another fragment: none
    F.append(([fwd(0, -3, 1)], [rev(MIN_INS, -5, 0), rev(MIN_INS - 1, -9, 1), rev(MAX_INS, -4, 2), rev(MAX_INS + 1, -2, 3)]))   # the bounds at either edge
    F.append(([(1300, 2, 1, 1, -1.75)], [(1300 + LEN - MAX_INS, 2, 0, 2, -2.25), (1300 + LEN - MAX_INS - 1, 2, 0, 0, 0.25)]))  # mate 2 forward
    F.append(([fwd(x, -x, x % 4) for x in range(4)], [rev(300 + y, 2 - 4 * y, y % 3) for y in range(8)]))                       # 32 cells: a lane
    F.append(([fwd(x, -x, x % 4) for x in range(3)], [rev(300 + y, 2 - 4 * y, y % 3) for y in range(11)]))                      # 33 cells: a wave
    F.append(([fwd(x, -40 + RISES[x % 10] * (x // 10 + 1), x % 5) for x in range(40)], [rev(320 + y, -y, y) for y in range(3)]))    # mate 1 the longer list
    F.append(([fwd(y, -y, y) for y in range(3)], [rev(320 + x, -40 + RISES[x % 10] * (x // 10 + 1), x % 5) for x in range(70)]))    # mate 2 the longer list
    F.append(([fwd(x, -7, 1) for x in range(20)], [rev(330 + y, -7, 1) for y in range(20)]))                                      # 400 equal pairs: saturation
    return F


def _pair_lists(frags):
    l1 = _lists([a for a, _ in frags])
    l2 = _lists([b for _, b in frags])
    n = len(frags)
    return l1[0], l1[1], np.full(n, LEN, dtype=np.uint32), l2[0], l2[1], np.full(n, LEN, dtype=np.uint32)


@pytest.mark.parametrize("scores", [1, 0])
def test_mapq_pair_hits_on_hand_made_lists(matchers, scores):
    import torch
    m = matchers[scores]
    frags = _pair_fragments()
    h1, o1, l1, h2, o2, l2 = L = _pair_lists(frags)
    accs = mq.check_pair_hits([(h1, o1, h2, o2)], l1, l2, MIN_INS, MAX_INS, scores)
    assert accs == mq.check_pair_hits_cellwise([(h1, o1, h2, o2)], l1, l2, MIN_INS, MAX_INS, scores, count=mq.sorted_acc_of_levels)
    assert [a["n"] for a in accs] == [0, 0, 0, 1, 0, 2, 1, 32, 33, 120, 210, 400], [a["n"] for a in accs]
    assert accs[11]["cnt"][0] == 255
    want = mq.acc_records(accs)
    m.mapq_stats(reset=True)
    _same(m.mapq_pair_hits(*L, MIN_INS, MAX_INS), want, "host lists")
    st = m.mapq_stats()
    cells = [len(a) * len(b) for a, b in frags]
    assert (st["folded"], st["candidates"], st["handed_over"], st["launches"]) == (len(frags), sum(cells), sum(c > 32 for c in cells), 2), st
    # the order of the hits; the lists of mate 1 in two blocks, both orders; device lists and records
    rng = np.random.default_rng(6)
    G = [([a[j] for j in rng.permutation(len(a))], [b[j] for j in rng.permutation(len(b))]) for a, b in frags]
    _same(m.mapq_pair_hits(*_pair_lists(G), MIN_INS, MAX_INS), want, "shuffled")
    A, B = _pair_lists([(a[:len(a) // 2], b) for a, b in frags]), _pair_lists([(a[len(a) // 2:], b) for a, b in frags])
    _same(m.mapq_pair_hits(*B, MIN_INS, MAX_INS, acc=m.mapq_pair_hits(*A, MIN_INS, MAX_INS)), want, "two blocks")
    _same(m.mapq_pair_hits(*A, MIN_INS, MAX_INS, acc=m.mapq_pair_hits(*B, MIN_INS, MAX_INS)), want, "two blocks, the other order")
    rec = torch.full((len(frags) * 40,), 0xAB, dtype=torch.uint8, device="cuda")
    m.mapq_pair_hits(*[_dev(x) for x in L], MIN_INS, MAX_INS, acc=rec, fresh=True)
    _same(rec.cpu().numpy(), want, "device lists")
    assert m.mapq_pair_hits(*_pair_lists([]), MIN_INS, MAX_INS).shape == (0,)


# ---- the finish on hand-made records -------------------------------------------------------------------------------------------
def _random_accs(rng, n, scores):
    """empty ones, crowded ones (low qualities), and ones with two or three candidates (the high qualities); with scores off the
    levels are those of mismatch counts: multiples of 12, at most 0"""
    step = 1 if scores else mq.MISMATCH_LEVELS
    out = []
    for _ in range(n):
        kind = rng.random()
        if kind < 0.1:
            out.append(mq.empty())
            continue
        if kind < 0.4:
            cnt = [int(c) for c in rng.choice([0, 0, 0, 0, 1, 1, 2, 9, 255], size=32)]
            cnt[0] = max(1, cnt[0])
        else:
            cnt = [1] + [0] * 31
            for j in rng.integers(1, 32 // step + (step > 1), size=int(rng.integers(0, 3))):
                cnt[int(j) * step] += 1
        level = int(rng.integers(-60, 10)) if scores else -step * int(rng.integers(0, 4))
        out.append({"level": level, "n": int(sum(cnt)) + int(rng.integers(0, 3)), "cnt": cnt})
    return out


def _placement_levels(rng, accs, scores):
    """a level per accumulator: half of them one of its candidates' (listed), the others anywhere from above its top to below its
    window (scores off: a multiple of 12, at most 0)"""
    step = 1 if scores else mq.MISMATCH_LEVELS
    lv = np.array([a["level"] if a["n"] else 0 for a in accs], dtype=np.int64) - step * rng.integers(-2, 34 // step + 1, size=len(accs))
    for i, a in enumerate(accs):
        held = [j for j, c in enumerate(a["cnt"]) if c and j % step == 0]
        if a["n"] and i % 2:
            lv[i] = a["level"] - held[int(rng.integers(0, len(held)))]
    return np.minimum(lv, 0) if not scores else lv


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("n", [0, 1, 65, 300])
def test_finish_single_end(matchers, scores, n):
    m = matchers[scores]
    rng = np.random.default_rng(20 + n)
    accs = _random_accs(rng, n, scores)
    state = np.arange(n) % 5                                                             # every state: only 1 and 2 place
    err = rng.integers(0, 6, size=n)                                                     # (scores on: the errors field plays no part)
    lv = _placement_levels(rng, accs, scores)
    if not scores:
        err = -lv // mq.MISMATCH_LEVELS
    score = (lv / 2 + 0.25).astype(np.float32)
    info = ((state.astype(np.uint64) << np.uint64(61)) | (np.uint64(7) << np.uint64(45)) | (err.astype(np.uint64) << np.uint64(41)) |
            (np.uint64(5) << np.uint64(35)) | np.uint64(123456))                         # (another file id than any text's: it plays no part)
    want, placed, unl = mq.finish_single(state, err, score, accs, scores)
    rec = mq.acc_records(accs)
    m.mapq_stats(reset=True)
    got = m.mapq(info, score if scores else None, rec)
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), np.nonzero(got != want)[0][:5]
    st = m.mapq_stats()
    assert (st["placements"], st["unlisted"], st["launches"]) == (placed, unl, 1 if n else 0), (st, placed, unl)
    if n >= 65:
        assert unl >= 3 and placed - unl >= 3 and len(set(int(q) for q in want)) >= (9 if scores and n == 300 else 4)      # both kinds, many values
        d = m.mapq(_dev(info), _dev(score), _dev(rec))
        assert d.cpu().numpy().tobytes() == want.tobytes()


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("n", [1, 65, 300])
def test_finish_pairs(matchers, scores, n):
    m = matchers[scores]
    rng = np.random.default_rng(40 + n)
    accp, acc1, acc2 = (_random_accs(rng, n, scores) for _ in range(3))
    pairs, s1, s2 = new_pair_info(n), new_single_info(n), new_single_info(n)
    pairs["state"] = (np.arange(n) // 3) % 3                                             # every state of the pair, under every state of the singles
    pairs["fileid"], pairs["pos1"], pairs["pos2"] = 3, 1000, 1200
    pairs["k1"], pairs["k2"] = rng.integers(0, 4, size=n), rng.integers(0, 4, size=n)
    lv = _placement_levels(rng, accp, scores)
    pairs["best"] = np.where(pairs["state"] == 0, -np.inf, lv / 2 + 0.25)
    if not scores:
        pairs["k1"] = -lv // mq.MISMATCH_LEVELS // 2
        pairs["k2"] = -lv // mq.MISMATCH_LEVELS - pairs["k1"]
        pairs["best"] = np.where(pairs["state"] == 0, -np.inf, -(pairs["k1"].astype(np.float64) + pairs["k2"]))
    for s, acc in ((s1, acc1), (s2, acc2)):
        st = (np.arange(n) + rng.integers(0, 3)) % 3
        k = rng.integers(0, 4, size=n)
        lvs = _placement_levels(rng, acc, scores)
        s["score"], s["pos"], s["fileid"] = (lvs / 2 + 0.25).astype(np.float32), 777, 2
        if not scores:
            k = -lvs // mq.MISMATCH_LEVELS
        s["tag"] = (k & 15) | ((np.arange(n) & 1) << 4) | (st << 5)
    R = [mq.acc_records(a) for a in (accp, acc1, acc2)]
    want, placed, unl = mq.finish_pairs(pairs, s1, s2, accp, acc1, acc2, scores)
    m.mapq_stats(reset=True)
    got = m.mapq_pairs(pairs, R[0], s1, s2, R[1], R[2])
    assert got.shape == (2 * n,) and got.tobytes() == want.tobytes(), np.nonzero(got != want)[0][:5]
    st = m.mapq_stats()
    assert (st["placements"], st["unlisted"]) == (placed, unl), (st, placed, unl)
    alone, placed0, _ = mq.finish_pairs(pairs, None, None, accp, None, None, scores)     # singles NULL: the pairs alone
    assert m.mapq_pairs(pairs, R[0]).tobytes() == alone.tobytes()
    if n >= 65:
        assert placed > placed0 > 0 and (alone != want).any() and (want[0::2] != want[1::2]).any()
        d = m.mapq_pairs(_dev(pairs), _dev(R[0]), _dev(s1), _dev(s2), _dev(R[1]), _dev(R[2]))
        assert d.cpu().numpy().tobytes() == want.tobytes()


def test_mapq_errors_are_loud(matchers):
    m = matchers[1]
    INV, OK = rlib.REAL_HIP_E_INVALID, rlib.REAL_HIP_OK
    h, off = _lists(_reads(20))
    acc, out = new_mapq_acc(20), np.zeros(40, dtype=np.uint8)
    L = m._L
    assert L.real_hip_mapq_hits(m._h, h.ctypes.data, off.ctypes.data, 20, 0, 1, acc.ctypes.data) == OK
    assert L.real_hip_mapq_hits(m._h, h.ctypes.data, off.ctypes.data, 20, 0, 1, None) == INV
    assert L.real_hip_mapq_hits(m._h, h.ctypes.data, None, 20, 0, 1, acc.ctypes.data) == INV
    assert L.real_hip_mapq_hits(m._h, None, off.ctypes.data, 20, 0, 1, acc.ctypes.data) == INV               # a null list with hits
    assert L.real_hip_mapq_hits(m._h, h.ctypes.data, off.ctypes.data, 1 << 32, 0, 1, acc.ctypes.data) == INV
    bad = off.copy()
    bad[5] = bad[6] + 1
    assert L.real_hip_mapq_hits(m._h, h.ctypes.data, bad.ctypes.data, 20, 0, 1, acc.ctypes.data) == INV      # offsets running backwards
    assert L.real_hip_mapq_hits(m._h, None, None, 0, 0, 1, None) == OK                                        # no reads: nothing to do
    pp = PairMatcher._pair_params(MIN_INS, MAX_INS)
    P = _pair_lists(_pair_fragments()[:8])
    ptr = [x.ctypes.data for x in P]
    assert L.real_hip_mapq_pair_hits(m._h, C.byref(pp), *ptr, 8, 0, 1, acc.ctypes.data) == OK
    assert L.real_hip_mapq_pair_hits(m._h, C.byref(pp), *ptr, 8, 0, 1, None) == INV
    assert L.real_hip_mapq_pair_hits(m._h, C.byref(pp), *ptr[:2], None, *ptr[3:], 8, 0, 1, acc.ctypes.data) == INV
    assert L.real_hip_mapq_pair_hits(m._h, None, *ptr, 8, 0, 1, acc.ctypes.data) == INV
    rev = PairMatcher._pair_params(MAX_INS, MIN_INS)
    assert L.real_hip_mapq_pair_hits(m._h, C.byref(rev), *ptr, 8, 0, 1, acc.ctypes.data) == INV
    assert L.real_hip_mapq_pair_hits(m._h, C.byref(pp), *([None] * 6), 0, 0, 1, None) == OK
    info, score = np.zeros(20, dtype=np.uint64), np.zeros(20, dtype=np.float32)
    assert L.real_hip_mapq(m._h, info.ctypes.data, score.ctypes.data, acc.ctypes.data, 20, 0, out.ctypes.data) == OK
    assert L.real_hip_mapq(m._h, None, score.ctypes.data, acc.ctypes.data, 20, 0, out.ctypes.data) == INV
    assert L.real_hip_mapq(m._h, info.ctypes.data, None, acc.ctypes.data, 20, 0, out.ctypes.data) == INV      # scores on: the level comes from the score
    assert L.real_hip_mapq(m._h, info.ctypes.data, score.ctypes.data, None, 20, 0, out.ctypes.data) == INV
    assert L.real_hip_mapq(m._h, info.ctypes.data, score.ctypes.data, acc.ctypes.data, 20, 0, None) == INV
    assert L.real_hip_mapq(m._h, info.ctypes.data, score.ctypes.data, acc.ctypes.data, 1 << 32, 0, out.ctypes.data) == INV
    assert L.real_hip_mapq(m._h, None, None, None, 0, 0, None) == OK
    pairs, sg = new_pair_info(20), new_single_info(20)
    a = acc.ctypes.data
    assert L.real_hip_mapq_pairs(m._h, pairs.ctypes.data, sg.ctypes.data, sg.ctypes.data, a, a, a, 20, 0, out.ctypes.data) == OK
    assert L.real_hip_mapq_pairs(m._h, pairs.ctypes.data, None, None, a, None, None, 20, 0, out.ctypes.data) == OK
    assert L.real_hip_mapq_pairs(m._h, pairs.ctypes.data, sg.ctypes.data, None, a, a, a, 20, 0, out.ctypes.data) == INV     # one singles pointer without the other
    assert L.real_hip_mapq_pairs(m._h, pairs.ctypes.data, None, sg.ctypes.data, a, a, a, 0, 0, out.ctypes.data) == INV      # also with nothing to do
    assert L.real_hip_mapq_pairs(m._h, pairs.ctypes.data, sg.ctypes.data, sg.ctypes.data, a, None, a, 20, 0, out.ctypes.data) == INV
    assert L.real_hip_mapq_pairs(m._h, None, None, None, a, None, None, 20, 0, out.ctypes.data) == INV
    assert L.real_hip_mapq_pairs(m._h, pairs.ctypes.data, None, None, None, None, None, 20, 0, out.ctypes.data) == INV
    assert L.real_hip_mapq_pairs(m._h, pairs.ctypes.data, None, None, a, None, None, 20, 0, None) == INV
    assert L.real_hip_mapq_pairs(m._h, pairs.ctypes.data, None, None, a, None, None, 1 << 32, 0, out.ctypes.data) == INV
    st = rlib.RealHipMapqStats()
    st.struct_size = C.sizeof(rlib.RealHipMapqStats) - 8
    assert L.real_hip_mapq_stats_get(m._h, C.byref(st), 0) == INV
    # batches that disagree, null accumulators, no text: real_hip_match_mapq / _pairs_mapq
    b = m._read_batch(np.zeros(200, dtype=np.uint8), np.zeros(200, dtype=np.uint8), patl=100)
    b3 = m._read_batch(np.zeros(300, dtype=np.uint8), np.zeros(300, dtype=np.uint8), patl=100)
    assert L.real_hip_match_mapq(m._h, C.byref(b), acc.ctypes.data) == rlib.REAL_HIP_E_STATE                 # neither text nor index
    assert L.real_hip_match_mapq(m._h, None, acc.ctypes.data) == INV
    args = (pairs.ctypes.data, sg.ctypes.data, sg.ctypes.data, a, a, a)
    assert L.real_hip_match_pairs_mapq(m._h, C.byref(b), C.byref(b3), C.byref(pp), None, *args) == INV
    assert L.real_hip_match_pairs_mapq(m._h, C.byref(b), C.byref(b), C.byref(pp), None, *args[:5], None) == INV
    assert L.real_hip_match_pairs_mapq(m._h, C.byref(b), C.byref(b), C.byref(pp), None, *args[:2], None, *args[3:]) == INV
    assert L.real_hip_match_pairs_mapq(m._h, C.byref(b), C.byref(b), C.byref(rev), None, *args) == INV
    # the context still works
    _same(m.mapq_hits(h, off), mq.acc_records(mq.check_hits([(h, off)], 20, 1)), "after the errors")


# ---- the whole path ---------------------------------------------------------------------------------------------------------
def _matcher(g, case):
    scores, tk, fl, seedl, _, _, tkind, pb = case
    m = PairMatcher(_opts(seedl, tk, scores, fl), prefix_bits=pb, table_kind=tkind)
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    return m


@pytest.mark.parametrize("case", mw.CASES)
@pytest.mark.parametrize("kind", mw.KINDS)
def test_match_mapq_against_the_checker(ora, kind, case):
    import torch
    w = mw.workload(ora, kind, case)
    print(kind, case, w["cov"], w["longer_than_32"], w["products_beyond_32"], w["placements"])
    mw.assert_coverage(w, kind)
    scores, b1, b2, n = case[0], w["b1"], w["b2"], w["b1"].n_reads
    want = [mq.acc_records(w[k]) for k in ("accp", "acc1", "acc2")]
    m = _matcher(w["g"], case)
    plain = m.match_pairs_singles(b1, b2, pw.MIN_INS, pw.MAX_INS)
    m.mapq_stats(reset=True)
    got = m.match_pairs_mapq(b1, b2, pw.MIN_INS, pw.MAX_INS)
    st = m.mapq_stats()
    for k in range(3):                                      # pairs and singles: bit for bit what real_hip_match_pairs_singles gives
        assert got[k].tobytes() == plain[k].tobytes(), k
    for k, name in enumerate(("the pairs", "mate 1", "mate 2")):
        _same(got[3 + k], want[k], "%s %s %r" % (name, kind, case))
    assert (st["folded"], st["candidates"], st["handed_over"], st["launches"]) == (
        3 * n, w["hits"] + w["products"], w["longer_than_32"] + w["products_beyond_32"], 4), (st, w["hits"], w["products"])
    # the finish: with the singles, and the pairs alone
    m.mapq_stats(reset=True)
    q = m.mapq_pairs(got[0], got[3], got[1], got[2], got[4], got[5])
    assert q.tobytes() == w["mapq"].tobytes(), np.nonzero(q != w["mapq"])[0][:5]
    st = m.mapq_stats()
    assert (st["placements"], st["unlisted"]) == (w["placements"], 0), st
    assert m.mapq_pairs(got[0], got[3]).tobytes() == w["mapq_pairs_only"].tobytes()
    # the same file again into the accumulators (fresh = 0): every candidate twice; pairs and singles do not change
    again = m.match_pairs_mapq(b1, b2, pw.MIN_INS, pw.MAX_INS, *[x.copy() for x in got])
    for k in range(3):
        assert again[k].tobytes() == plain[k].tobytes(), k
        _same(again[3 + k], mq.acc_records([mq.merge(a, a) for a in w[("accp", "acc1", "acc2")[k]]]), "folded twice")
    # batches and outputs on the device
    dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)]
    outs = [torch.full((n * size,), 0xCD, dtype=torch.uint8, device="cuda") for size in (40, 16, 16, 40, 40, 40)]
    m.match_pairs_mapq(dev[0], dev[1], pw.MIN_INS, pw.MAX_INS, *outs, fresh=True)
    for k in range(3):
        assert outs[k].cpu().numpy().tobytes() == plain[k].tobytes(), k
        _same(outs[3 + k].cpu().numpy(), want[k], "device outputs")
    dq = m.mapq_pairs(outs[0], outs[3], outs[1], outs[2], outs[4], outs[5])
    assert dq.cpu().numpy().tobytes() == w["mapq"].tobytes()
    # single-end: mate 1's reads alone, the finish over the records of real_hip_match_unique
    m.mapq_stats(reset=True)
    acc = m.match_mapq(b1.bases, b1.qual, b1.offsets)
    _same(acc, want[1], "real_hip_match_mapq")
    st = m.mapq_stats()
    assert (st["folded"], st["candidates"], st["launches"]) == (n, int(w["f"][2][-1]), 2), st
    _same(m.match_mapq(b1.bases, b1.qual, b1.offsets, acc=acc.copy()), mq.acc_records([mq.merge(a, a) for a in w["acc1"]]), "match_mapq folded twice")
    info, score = m.match_unique(b1.bases, b1.qual, b1.offsets, fresh=True)
    state, _, err, _, _ = unpack_info(info)
    want_q, placed, unl = mq.finish_single(state, err, score, w["acc1"], scores)
    q1 = m.mapq(info, score, acc)
    assert q1.tobytes() == want_q.tobytes() and placed > n // 4 and unl == 0
    dacc = torch.full((n * 40,), 0xCD, dtype=torch.uint8, device="cuda")
    m.match_mapq(*dev[0], acc=dacc, fresh=True)
    _same(dacc.cpu().numpy(), want[1], "real_hip_match_mapq, device")
    m.close()


def test_match_pairs_mapq_with_the_mate_search(ora):
    """with sp the pairs are real_hip_match_pairs_search's, the accumulators stay folds of seed hits, and the placements only the
    search found arrive as unlisted at the finish"""
    scores, tk, fl, seedl = 1, 3, 2, 32
    g, b1, b2, planted = msw.search_workload("iid", False, (100, 80), seedl, tk)
    _, h1, o1, h2, o2 = msw.oracle_lists(ora, g, b1, b2, seedl, tk, scores, fl)
    n, l1, l2 = b1.n_reads, msw.lens_of(b1), msw.lens_of(b2)
    accp = mq.check_pair_hits([(h1, o1, h2, o2)], l1, l2, msw.MIN_INS, msw.MAX_INS, scores)
    acc1, acc2 = mq.check_hits([(h1, o1)], n, scores), mq.check_hits([(h2, o2)], n, scores)
    m = _matcher(g, (scores, tk, fl, seedl, False, None, 0, 0))
    plain = m.match_pairs_singles(b1, b2, msw.MIN_INS, msw.MAX_INS, mate_search=True)
    got = m.match_pairs_mapq(b1, b2, msw.MIN_INS, msw.MAX_INS, mate_search=True)
    for k in range(3):
        assert got[k].tobytes() == plain[k].tobytes(), k
    for k, a in enumerate((accp, acc1, acc2)):
        _same(got[3 + k], mq.acc_records(a), "accumulators with the search")
    want, placed, unl = mq.finish_pairs(plain[0], plain[1], plain[2], accp, acc1, acc2, scores)
    rescued = [i for i in planted["A"] if plain[0]["state"][i] == 1]
    assert len(rescued) >= 4 and unl >= 2 * len(rescued) and all(accp[i]["n"] == 0 and want[2 * i] == 60 for i in rescued), (rescued, unl)
    m.mapq_stats(reset=True)
    q = m.mapq_pairs(got[0], got[3], got[1], got[2], got[4], got[5])
    assert q.tobytes() == want.tobytes()
    st = m.mapq_stats()
    assert (st["placements"], st["unlisted"]) == (placed, unl) and st["unlisted"] > 0, st
    m.close()
