"""The library's host layer: an array that crosses the ABI is host memory (staged in the context's buffers, downloaded
afterwards) or device memory (used where it lies), and the two must give the same bytes; the staging buffers are reused from
call to call; every paired stage keeps its own counts.  Nothing here knows what the right records are -- the stages have
their checkers elsewhere -- only that the same inputs give the same outputs whichever side they come from and whatever the
context did before."""
import ctypes as C
import types

import numpy as np
import pytest

import pairs_workloads as pw
from real_amd import lib as rlib
from real_amd.matcher import PairMatcher, RealOptions

pytestmark = pytest.mark.gpu
SEEDL, TOTALK, FILTER_LEVEL = 32, 3, 2
N_BINS = pw.MAX_INS + 2
SIZES = [1, 65, 300]               # one lane; one wave and one; more than one block of 256
SEQUENCE = [300, 1, 65, 300]       # the buffers shrink, grow and come back to a size they had
CALLS = ("unique", "all1", "all2", "pair_hits", "single_hits", "insert_hist", "pair_all_hits", "match_pairs_singles")


@pytest.fixture(scope="module")
def load():
    """the genome (6000 bases, four fragments) and, per n, the two mates' batches: half of the fragments have reads of
    100 / 80 bases, the other half ragged ones (n = 1: a ragged one)"""
    import torch
    torch.zeros(1, device="cuda")      # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    g, b1, b2 = pw.pair_workload("iid", True, n=300, size=6000)
    assert b1.n_reads == 450

    def part(b, n):
        lo = 300 - n // 2
        o = b.offsets[lo:lo + n + 1]
        return types.SimpleNamespace(n_reads=n, bases=b.bases[int(o[0]):int(o[-1])].copy(), qual=b.qual[int(o[0]):int(o[-1])].copy(),
                                     offsets=(o - o[0]).astype(np.uint64))
    return g, {n: (part(b1, n), part(b2, n)) for n in SIZES}


def _matcher(g):
    m = PairMatcher(RealOptions(seedl=SEEDL, seedkmax=2, totalkmax=TOTALK, scores=True, filter_level=FILTER_LEVEL).normalise())
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    return m


def _junk(n, dtype, seed):
    """n records of arbitrary bytes: what an output-only array may hold before the call"""
    return np.random.default_rng(seed).integers(0, 256, size=n * np.dtype(dtype).itemsize, dtype=np.uint8).view(dtype)


def _dev(a):
    """the same bytes as a device tensor: one element per item of a plain array (the wrappers count them), bytes of records"""
    import torch
    a = np.ascontiguousarray(a)
    word = np.uint8 if a.dtype.fields else {1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(word).copy()).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(np.uint8).view(dtype)


def _match_all_device(m, b, cap):
    """real_hip_match_all with a device batch and device outputs: HipMatcher.match_all takes host batches only, so this
    side goes through the ABI as test_gpu_pipeline.py does"""
    db = (_dev(b.bases), _dev(b.qual), _dev(b.offsets))
    hits = _dev(_junk(max(cap, 1), rlib.HIT_DTYPE, 5))
    hoff = _dev(_junk(b.n_reads + 1, np.uint64, 6))
    batch = m._batch(db[0], db[1], db[2], 0, None)
    nout = C.c_uint64(0)
    m.sync_inputs(*db, hits, hoff)
    m._check(m._L.real_hip_match_all(m._h, C.byref(batch), hits.data_ptr(), cap, C.byref(nout), hoff.data_ptr()))
    return _host(hits, rlib.HIT_DTYPE)[:int(nout.value)], _host(hoff, np.uint64)


def _run(m, mates, device, prev=None):
    """the seven entry points on one pair of batches -> {call: bytes of its outputs}.  prev: the outputs of an earlier _run
    to fold into; without it every in/out array starts as junk and the call is `fresh`.  match_all, pair_all_hits: output
    only, they have no fold."""
    b1, b2 = mates
    n = b1.n_reads
    fresh = prev is None
    l1, l2 = pw.lens_of(b1), pw.lens_of(b2)
    side = _dev if device else (lambda a: np.ascontiguousarray(a).copy())
    back = _host if device else (lambda a, dtype: a.view(dtype))

    def start(call, k, dtype, count=n):
        """in/out array k of `call`: junk, or what the earlier run left"""
        return side(_junk(count, dtype, 7 + k) if fresh else np.frombuffer(prev[call][k], dtype=dtype))

    def dev_batch(b):
        return (_dev(b.bases), _dev(b.qual), _dev(b.offsets)) if device else b

    out = {}
    d1 = dev_batch(b1)
    info, score = start("unique", 0, np.uint64), start("unique", 1, np.float32)
    m.match_unique(*(d1 if device else (b1.bases, b1.qual, b1.offsets)), info=info, score=score, fresh=fresh)
    out["unique"] = (back(info, np.uint64).tobytes(), back(score, np.float32).tobytes())

    lists = []
    for k, b in enumerate((b1, b2)):
        if device:
            h, o = _match_all_device(m, b, cap=max(1024, 4 * n))
        else:
            h, o = m.match_all(b.bases, b.qual, b.offsets)
        out["all%d" % (k + 1)] = (h.tobytes(), o.tobytes())
        lists.append((h, o))
    (h1, o1), (h2, o2) = lists
    L = [side(x) for x in (h1, o1, l1, h2, o2, l2)]

    pairs = start("pair_hits", 0, rlib.PAIR_DTYPE)
    m.pair_hits(*L, pw.MIN_INS, pw.MAX_INS, fileid=0 if fresh else 1, pairs=pairs, fresh=fresh)
    out["pair_hits"] = (back(pairs, rlib.PAIR_DTYPE).tobytes(),)

    singles = start("single_hits", 0, rlib.SINGLE_DTYPE)
    m.single_hits(L[0], L[1], L[2], fileid=0 if fresh else 1, singles=singles, fresh=fresh)
    out["single_hits"] = (back(singles, rlib.SINGLE_DTYPE).tobytes(),)

    hist = start("insert_hist", 0, np.uint64, N_BINS)
    m.insert_hist(pairs, L[2], L[5], N_BINS, hist=hist, fresh=fresh)
    out["insert_hist"] = (back(hist, np.uint64).tobytes(),)

    if device:
        ph, po = _dev(_junk(4096, rlib.PAIR_HIT_DTYPE, 20)), _dev(_junk(n + 1, np.uint64, 21))
        found, _ = m.pair_all_hits(*L, pw.MIN_INS, pw.MAX_INS, out=ph, pair_offsets=po)
        ph, po = _host(ph, rlib.PAIR_HIT_DTYPE)[:found], _host(po, np.uint64)
    else:
        ph, po = m.pair_all_hits(*L, pw.MIN_INS, pw.MAX_INS, cap=4096)
    out["pair_all_hits"] = (ph.tobytes(), po.tobytes())

    rec = [start("match_pairs_singles", 0, rlib.PAIR_DTYPE), start("match_pairs_singles", 1, rlib.SINGLE_DTYPE),
           start("match_pairs_singles", 2, rlib.SINGLE_DTYPE)]
    m.match_pairs_singles(d1, dev_batch(b2), pw.MIN_INS, pw.MAX_INS, pairs=rec[0], singles1=rec[1], singles2=rec[2], mate_search=True, fresh=fresh)
    out["match_pairs_singles"] = tuple(back(r, dt).tobytes() for r, dt in zip(rec, (rlib.PAIR_DTYPE, rlib.SINGLE_DTYPE, rlib.SINGLE_DTYPE)))
    assert set(out) == set(CALLS)
    return out


def _same(got, want, what):
    for call in CALLS:
        for k, (x, y) in enumerate(zip(got[call], want[call])):
            assert len(got[call]) == len(want[call]) and x == y, "%s: %s, array %d differs" % (what, call, k)


_fresh_host = {}                   # n -> what a new context gives for host arrays (shared with the reuse test)


def _reference(load, n):
    if n not in _fresh_host:
        g, mates = load
        m = _matcher(g)
        _fresh_host[n] = _run(m, mates[n], device=False)
        m.close()
    return _fresh_host[n]


@pytest.mark.parametrize("n", SIZES)
def test_host_arrays_equal_device_arrays(load, n):
    g, mates = load
    m = _matcher(g)
    host = _run(m, mates[n], device=False)
    _fresh_host.setdefault(n, host)
    dev = _run(m, mates[n], device=True)
    _same(dev, host, "n = %d, fresh, device against host" % n)
    # what the calls found is not nothing: reads matched, fragments paired, the histogram counted (n = 1: one fragment)
    hits, pairs = np.frombuffer(host["all1"][0], dtype=rlib.HIT_DTYPE), np.frombuffer(host["pair_hits"][0], dtype=rlib.PAIR_DTYPE)
    unique = int((pairs["state"] == 1).sum())
    print("n = %d: %d hits of mate 1, %d fragments paired, %d of them Unique" % (n, len(hits), int((pairs["state"] != 0).sum()), unique))
    assert int(np.frombuffer(host["insert_hist"][0], dtype=np.uint64).sum()) == unique
    if n > 1:      # (the reads are samples of the genome with 1 % of errors: most are found, most fragments pair)
        assert len(hits) >= n // 2 and unique >= n // 4
    # folding into the records of the call before: uploaded on the host side, read in place on the device side
    host2 = _run(m, mates[n], device=False, prev=host)
    dev2 = _run(m, mates[n], device=True, prev=host)
    _same(dev2, host2, "n = %d, fold, device against host" % n)
    # (the earlier counts were read: the Unique records of this call came on top of them; and the records of file 0 met the
    # same placements in file 1)
    h1, h2 = (np.frombuffer(o["insert_hist"][0], dtype=np.uint64).astype(np.int64) for o in (host, host2))
    unique2 = int((np.frombuffer(host2["pair_hits"][0], dtype=rlib.PAIR_DTYPE)["state"] == 1).sum())
    assert (h2 >= h1).all() and int((h2 - h1).sum()) == unique2
    if n > 1:
        assert host2["pair_hits"][0] != host["pair_hits"][0] and host2["single_hits"][0] != host["single_hits"][0]
    m.close()


@pytest.fixture(scope="module")
def reused(load):
    """one context through SEQUENCE with host arrays -> (matcher, the outputs of every step)"""
    g, mates = load
    m = _matcher(g)
    print("after the index build:", {k: v for k, v in m.index_build_stats().items() if k.startswith("alloc")})
    outs = [_run(m, mates[n], device=False) for n in SEQUENCE]
    print("after the sequence:", {k: v for k, v in m.index_build_stats().items() if k.startswith("alloc")})
    yield m, outs
    m.close()


def test_buffers_are_reused_across_sizes(load, reused):
    _, outs = reused
    for step, (n, got) in enumerate(zip(SEQUENCE, outs)):
        _same(got, _reference(load, n), "step %d of the sequence, n = %d, against a new context" % (step, n))


def test_stage_statistics(load, reused):
    m, outs = reused
    total = sum(SEQUENCE)
    hits = [sum(len(o["all%d" % k][0]) for o in outs) // rlib.HIT_DTYPE.itemsize for k in (1, 2)]
    unique = sum(int((np.frombuffer(o["pair_hits"][0], dtype=rlib.PAIR_DTYPE)["state"] == 1).sum()) for o in outs)
    pair_hits = sum(len(o["pair_all_hits"][0]) for o in outs) // rlib.PAIR_HIT_DTYPE.itemsize
    steps = len(SEQUENCE)
    # per step: the join runs twice (pair_hits, match_pairs_singles), the fold over one list and over two, the search, the
    # histogram and the enumeration once
    want = {
        "pair_stats": ({"pairs": 2 * total}, None),
        "mate_search_stats": ({"fragments": total}, 1 * steps),
        "single_stats": ({"reads": 3 * total, "hits": 2 * hits[0] + hits[1]}, 2 * 2 * steps),
        "insert_stats": ({"records": total, "counted": unique, "overflow": 0, "invalid": 0}, 1 * steps),
        "pair_all_stats": ({"fragments": total, "pairs_out": pair_hits}, None),
    }
    for name, (fields, launches) in want.items():
        st = getattr(m, name)()
        print(name, st)
        assert {k: st[k] for k in fields} == fields, (name, st)
        if "launches" in st:
            assert st["launches"] > 0 and st["kernel_ms"] > 0, (name, st)
            assert launches is None or st["launches"] == launches, (name, st)
        if name in ("pair_stats", "pair_all_stats"):
            assert st["products"] >= unique, (name, st)
        assert getattr(m, name)(reset=True) == st, name                # the same values once more ...
        again = getattr(m, name)()
        assert all(v == 0 for v in again.values()), (name, again)      # ... and then zeros
    # the join's two kernels are timed under their public ids: once per join each
    for which in (rlib.K_PAIR, rlib.K_PAIR_WAVE):
        ms, launched = m.kernel_time(which)
        assert launched == 2 * steps and ms > 0, (which, ms, launched)
    # the other stages start again from zero
    _run(m, load[1][65], device=False)
    assert m.insert_stats()["records"] == 65 and m.single_stats()["reads"] == 3 * 65 and m.pair_stats()["pairs"] == 2 * 65
    assert m.mate_search_stats()["launches"] == 1 and m.pair_all_stats()["fragments"] == 65
