"""The insert-size histogram on the device (real_hip_pair_insert_hist) against insert_checker.py, which restates the outer
distance, the overflow bin and the invalid rule in numpy and never calls the code under test.  Counts and statistics are
integers: everything is compared exactly."""
import ctypes as C

import numpy as np
import pytest

import insert_checker as ic
import insert_workloads as iw
import pairs_checker as pc
import pairs_workloads as pw
from real_amd import lib as rlib
from real_amd.matcher import PairMatcher, RealOptions

pytestmark = pytest.mark.gpu
BLOCK = 512                        # lanes of a block of the kernel
GRID = 256 * 2 * BLOCK             # records the grid covers in one stride: two blocks on each of the 256 CUs


def _opts(scores):
    return RealOptions(seedl=iw.SEEDL, seedkmax=2, totalkmax=iw.TOTALK, scores=bool(scores), filter_level=iw.FILTER_LEVEL).normalise()


@pytest.fixture(scope="module")
def m():
    import torch
    torch.zeros(1, device="cuda")      # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    x = PairMatcher(_opts(1))
    yield x
    x.close()


def _records(n, n_bins, seed, len_range=(30, 151)):
    """n records of all three states and both strands with ragged lengths: outer distances around and beyond n_bins, some
    exactly n_bins - 2 and n_bins - 1, forward positions small and just below 2^32 (the reverse mate then ends beyond 2^32),
    about 3 % invalid; the fields the histogram must not look at hold junk"""
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, dtype=rlib.PAIR_DTYPE)
    l1 = rng.integers(*len_range, size=n).astype(np.uint32)
    l2 = rng.integers(*len_range, size=n).astype(np.uint32)
    rec["state"] = rng.choice([pc.NOMATCH, pc.UNIQUE, pc.UNIQUE, pc.UNIQUE, pc.NONUNIQUE], size=n)
    rec["inverted1"] = rng.integers(0, 2, size=n)
    lr = np.where(rec["inverted1"] == 0, l2, l1).astype(np.int64)
    outer = np.maximum(lr, rng.normal(0.7 * n_bins, 0.25 * n_bins + 2, size=n).astype(np.int64))
    edge = rng.integers(0, 8, size=n)
    outer = np.where((edge == 0) & (lr <= n_bins - 2), n_bins - 2, outer)
    outer = np.where((edge == 1) & (lr <= n_bins - 1), n_bins - 1, outer)
    outer = np.where(edge == 2, lr, outer)                       # both mates start at one position
    gap = outer - lr
    fp = np.where(rng.integers(0, 2, size=n) == 0, rng.integers(0, 1 << 20, size=n), (1 << 32) - 1 - gap - rng.integers(0, 40, size=n))
    rp = fp + gap
    assert (fp >= 0).all() and (rp < (1 << 32)).all()
    bad = rng.integers(0, 33, size=n) == 0                       # invalid: the two positions swapped (where they differ)
    fp, rp = np.where(bad, rp, fp), np.where(bad, fp, rp)
    fwd1 = rec["inverted1"] == 0
    rec["pos1"], rec["pos2"] = np.where(fwd1, fp, rp), np.where(fwd1, rp, fp)
    rec["best"], rec["second"] = rng.normal(size=n), np.nan
    rec["score1"], rec["score2"] = rng.normal(size=n), np.inf
    rec["frag"], rec["fileid"], rec["k1"], rec["k2"], rec["reserved"] = rng.integers(0, 1 << 16, size=n), 255, 255, 255, 255
    return rec, l1, l2


def _dev(rec, l1, l2):
    import torch
    return (torch.from_numpy(rec.view(np.uint8).copy()).cuda(), torch.from_numpy(l1.view(np.int32).copy()).cuda(),
            torch.from_numpy(l2.view(np.int32).copy()).cuda())


def _check(m, rec, l1, l2, n_bins, what, device=True):
    import torch
    want, wst = ic.histogram(rec, l1, l2, n_bins)
    m.insert_stats(reset=True)
    got = m.insert_hist(rec, l1, l2, n_bins)
    st = m.insert_stats()
    assert got.dtype == np.uint64 and (got == want).all(), (what, np.nonzero(got != want)[0][:10])
    assert {k: st[k] for k in wst} == wst and st["launches"] == (1 if len(rec) else 0), (what, st, wst)
    assert int(got.sum()) == wst["counted"] and int(got[-1]) == wst["overflow"]
    if device:
        hist = torch.full((n_bins,), -7, dtype=torch.int64, device="cuda")       # fresh: output only, whatever it held
        m.insert_hist(*_dev(rec, l1, l2), n_bins, hist=hist, fresh=True)
        assert (hist.cpu().numpy().view(np.uint64) == want).all(), what + ", device pointers"
        st = m.insert_stats(reset=True)
        assert {k: st[k] for k in wst} == {k: 2 * v for k, v in wst.items()}, (what, st)
    return want, wst


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 4 * BLOCK + 3])
def test_insert_hist_record_counts(m, n):
    rec, l1, l2 = _records(n, 1002, seed=100 + n)
    want, wst = _check(m, rec, l1, l2, 1002, "n = %d" % n)
    if n >= 63:
        assert wst["invalid"] > 0 and wst["overflow"] > 0 and want[1000] > 0 and wst["counted"] < n - wst["invalid"]


@pytest.mark.parametrize("n_bins", [2, 3, 700, 1002, 16383, 16384])
def test_insert_hist_bin_counts(m, n_bins):
    """the two smallest histograms (lengths 0..2 there: an outer distance is at least the reverse mate's length), the default
    window's, and the largest"""
    rec, l1, l2 = _records(5000, n_bins, seed=n_bins, len_range=(0, 3) if n_bins < 100 else (30, 151))
    want, wst = _check(m, rec, l1, l2, n_bins, "n_bins = %d" % n_bins)
    assert want[n_bins - 2] > 0 and want[n_bins - 1] > 0 and want[0] > 0 if n_bins < 100 else want[n_bins - 2] > 50
    assert wst["invalid"] > 20 and (rec["pos1"] > 0xfff00000).sum() > 1000


def test_insert_hist_beyond_one_stride_of_the_grid(m):
    """more records than the grid covers in one stride, and than it covers in one turn of a lane's four records"""
    for n in (GRID + 777, 4 * GRID + 5):
        rec, l1, l2 = _records(n, 1002, seed=n)
        _check(m, rec, l1, l2, 1002, "n = %d" % n, device=(n < 2 * GRID))


def test_insert_hist_one_bin(m):
    rec, l1, l2 = _records(100_000, 1002, seed=9)
    rec["state"], rec["inverted1"] = pc.UNIQUE, 0
    rec["pos1"] = np.arange(100_000)
    rec["pos2"] = rec["pos1"] + 300 - l2
    want, wst = _check(m, rec, l1, l2, 1002, "one bin")
    assert int(want[300]) == 100_000 and wst == {"records": 100_000, "counted": 100_000, "overflow": 0, "invalid": 0}
    want, wst = _check(m, rec, l1, l2, 301, "one bin, the overflow bin")
    assert int(want[300]) == 100_000 and wst["overflow"] == 100_000


def test_insert_hist_accumulates(m):
    import torch
    a, b = _records(3000, 1002, seed=1), _records(1777, 1002, seed=2)
    whole = tuple(np.concatenate([x, y]) for x, y in zip(a, b))
    want, _ = ic.histogram(*whole, 1002)
    assert (m.insert_hist(*whole, 1002) == want).all()
    h = m.insert_hist(*a, 1002)
    h2 = m.insert_hist(*b, 1002, hist=h)
    assert h2 is h and (h == want).all()
    assert (m.insert_hist(*b, 1002, hist=m.insert_hist(*a, 1002)) == m.insert_hist(*a, 1002, hist=m.insert_hist(*b, 1002))).all()
    hist = torch.zeros(1002, dtype=torch.int64, device="cuda")
    m.insert_hist(*_dev(*a), 1002, hist=hist, fresh=True)
    m.insert_hist(*_dev(*b), 1002, hist=hist)
    assert (hist.cpu().numpy().view(np.uint64) == want).all()
    # no records: a fresh histogram is cleared, another one is left as it is
    none = tuple(x[:0] for x in a)
    junk = np.full(1002, 5, dtype=np.uint64)
    assert (m.insert_hist(*none, 1002, hist=junk.copy()) == 5).all() and (m.insert_hist(*none, 1002, hist=junk.copy(), fresh=True) == 0).all()
    m.insert_hist(*_dev(*none), 1002, hist=hist)
    assert (hist.cpu().numpy().view(np.uint64) == want).all()


def test_insert_hist_errors_are_loud(m):
    rec, l1, l2 = _records(100, 1002, seed=3)
    hist = np.zeros(16385, dtype=np.uint64)
    call = m._L.real_hip_pair_insert_hist
    ok = (rec.ctypes.data, l1.ctypes.data, l2.ctypes.data, 100, 0, 1)
    assert call(m._h, *ok, 1002, hist.ctypes.data) == rlib.REAL_HIP_OK
    for n_bins in (0, 1, rlib.REAL_HIP_INSERT_HIST_MAX_BINS + 1, 0xffffffff):
        assert call(m._h, *ok, n_bins, hist.ctypes.data) == rlib.REAL_HIP_E_INVALID, n_bins
    assert call(m._h, *ok, rlib.REAL_HIP_INSERT_HIST_MAX_BINS, hist.ctypes.data) == rlib.REAL_HIP_OK
    assert call(m._h, *ok, 1002, None) == rlib.REAL_HIP_E_INVALID
    assert call(m._h, None, *ok[1:], 1002, hist.ctypes.data) == rlib.REAL_HIP_E_INVALID
    assert call(m._h, ok[0], None, *ok[2:], 1002, hist.ctypes.data) == rlib.REAL_HIP_E_INVALID
    assert call(m._h, ok[0], ok[1], None, *ok[3:], 1002, hist.ctypes.data) == rlib.REAL_HIP_E_INVALID
    assert call(m._h, None, None, None, 0, 0, 1, 1002, hist.ctypes.data) == rlib.REAL_HIP_OK             # no records: nothing to read
    assert call(None, *ok, 1002, hist.ctypes.data) == rlib.REAL_HIP_E_INVALID
    st = rlib.RealHipInsertStats()
    st.struct_size = C.sizeof(rlib.RealHipInsertStats) - 8
    assert m._L.real_hip_insert_stats_get(m._h, C.byref(st), 0) == rlib.REAL_HIP_E_INVALID
    with pytest.raises(ValueError):
        m.insert_hist(rec, l1[:50], l2, 1002)
    with pytest.raises(ValueError):
        m.insert_hist(rec, l1, l2, 1002, hist=np.zeros(1001, dtype=np.uint64))
    _check(m, rec, l1, l2, 1002, "after the errors")               # the context still works


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("kind,ragged", iw.WORKLOADS)
def test_insert_hist_of_match_pairs_records(kind, ragged, scores):
    """the records real_hip_match_pairs leaves, on the host and left on the device, under the window 0..1000"""
    import torch
    g, b1, b2 = iw.workload(kind, ragged)
    mm = PairMatcher(_opts(scores))
    mm.set_text_symbols(0, g.sym, g.frag_start)
    mm.build_index_block()
    lo, hi = iw.WINDOW
    n, n_bins = b1.n_reads, hi + 2
    pairs = mm.match_pairs(b1, b2, lo, hi)
    l1, l2 = pw.lens_of(b1), pw.lens_of(b2)
    want, wst = _check(mm, pairs, l1, l2, n_bins, "%s scores %d" % (kind, scores))
    print(kind, ragged, scores, wst, "outers", np.nonzero(want)[0][[0, -1]])
    assert wst["counted"] == int((pairs["state"] == pc.UNIQUE).sum()) > 1000 and wst["invalid"] == 0 and wst["overflow"] == 0
    assert len(np.unique(l1)) > 1 or not ragged
    rc, est = ic.bounds(want)
    assert rc == 0 and PairMatcher.insert_bounds(want) == est and 250 < est["median"] < 350
    # the same without a download: batches, records, lengths and histogram stay on the device
    dev = [tuple(torch.from_numpy(x).cuda() for x in (b.bases, b.qual, b.offsets.view(np.int64))) for b in (b1, b2)]
    dp = torch.full((n * 40,), 0xCD, dtype=torch.uint8, device="cuda")
    mm.match_pairs(dev[0], dev[1], lo, hi, pairs=dp, fresh=True)
    dl = [(d[2][1:] - d[2][:-1]).to(torch.int32).contiguous() for d in dev]
    hist = torch.zeros(n_bins, dtype=torch.int64, device="cuda")
    mm.insert_hist(dp, dl[0], dl[1], n_bins, hist=hist, fresh=True)
    assert (hist.cpu().numpy().view(np.uint64) == want).all()
    assert mm.insert_bounds(hist) == est
    mm.close()
