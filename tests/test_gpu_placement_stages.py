"""The three stages that place reads on a text -- the pileup, the variant calls and the mismatch lists -- agree on WHICH records
they place: all three take a record to a placement with the one step of real_amd/csrc/read_walk.h (placed_read, on the
decoders of final_record.h).  The same hand-written records go through pileup_add, call_add on the finished pileup and
mismatches; `placed`, `other_file` and `invalid` of the three must be equal to each other and to tests/pileup_checker.py's.
With singles given, the mismatch lists place exactly the additional mates tests/sam_checker.py places.

One small text with an N run, set as file id 1, and 300 reads of 20 to 140 bases: more than a wave, more than the 256-thread
block of all three kernels, lengths on both sides of the walk's 32-, 64- and 128-base word boundaries.  No matcher, no
index, no oracle: the records are written by hand and cover what no matcher writes."""
import ctypes as C
import types

import numpy as np
import pytest

import pileup_checker as pk
import pileup_workloads as pw
import sam_checker as sk
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions, UniqueMatcher

pytestmark = pytest.mark.gpu

N, N_RUN, FILEID, READS = 3000, (1500, 1540), 1, 300
SHARED = ("placed", "other_file", "invalid")
CAP = 1 << 15                       # room for the lists of the pairs (a call that overflows is made again, and counts again)


def _info(state, pos, errors, fileid):
    return (state << 61) | (errors << 41) | (fileid << 35) | pos


@pytest.fixture(scope="module")
def case():
    """the text, the batch and its records, computed once and left unchanged"""
    rng = np.random.default_rng(20)
    sym = rng.integers(0, 4, size=N).astype(np.uint8)
    sym[N_RUN[0]:N_RUN[1]] = 4
    ref = np.where(sym > 3, 0, sym).astype(np.uint8)
    lens = rng.integers(20, 141, size=READS)
    lens[:12] = (20, 31, 32, 33, 63, 64, 65, 127, 128, 129, 139, 140)
    # single-end records: every state, file ids 0 / 1 / 2, both strands; positions that fit, then the ends of the range
    state = np.array([(1, 2, 1, 2, 0, 3, 4, 2, 1)[j % 9] for j in range(READS)])
    fileid = np.array([(1, 1, 1, 0, 1, 2, 1, 1)[j % 8] for j in range(READS)])
    pos = np.array([int(rng.integers(0, N - int(L) + 1)) for L in lens], dtype=np.int64)
    pos[270:280] = np.arange(N_RUN[0] - 40, N_RUN[0] - 30)              # (across the N run)
    special = {280: N - int(lens[280]), 281: N - int(lens[281]), 282: N - int(lens[282]) + 1, 283: N - int(lens[283]) + 1, 284: N, 285: N + 7,
               286: (1 << 32) + 5, 287: (1 << 33) + 5, 288: (1 << 32) + 5, 289: (1 << 35) - 1}
    for j, p in special.items():
        pos[j], state[j], fileid[j] = p, 1 + (j & 1), FILEID
    fileid[288] = 2                                                      # (another file comes before "behind the text")
    reads = []
    for j in range(READS):
        L, p = int(lens[j]), int(pos[j])
        o = ref[p:p + L].copy() if p + L <= N else rng.integers(0, 4, size=L).astype(np.uint8)
        o[::17] = (o[::17] + 1) & 3                                      # substitutions: sites for the calls, lists that are not empty
        reads.append(synth.revcomp(o) if state[j] == 2 else o)
    b = types.SimpleNamespace(bases=np.concatenate(reads), qual=None, offsets=np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64))
    info = np.array([_info(int(s), int(p), j % 16, int(f)) for j, (s, p, f) in enumerate(zip(state, pos, fileid))], dtype=np.uint64)
    # the same batch as both mates of 300 fragments: every pair state, both values of inverted1, the three file ids; mate 2 of
    # some ends one base behind the text
    pairs = np.zeros(READS, dtype=rlib.PAIR_DTYPE)
    pairs["state"] = [(1, 1, 0, 2, 1)[j % 5] for j in range(READS)]
    pairs["inverted1"] = [(j // 5) & 1 for j in range(READS)]
    pairs["fileid"] = [(1, 1, 1, 1, 0, 1, 2)[j % 7] for j in range(READS)]
    pairs["pos1"] = [int(p) & 0xffffffff for p in pos]
    pairs["pos2"] = [N - int(L) + (1 if j % 11 == 0 else 0) for j, L in enumerate(lens)]
    pairs["k1"], pairs["k2"] = 3, 5
    singles = []
    for m in (0, 1):
        s = np.zeros(READS, dtype=rlib.SINGLE_DTYPE)
        q = np.arange(READS) // 5 + m                                    # (apart from the pair states, which go by j % 5)
        s["pos"] = [int(rng.integers(0, N - int(L) + 1)) + (N if q[j] % 3 == 0 else 0) for j, L in enumerate(lens)]
        s["fileid"] = [(1, 1, 2, 1, 0)[q[j] % 5] for j in range(READS)]
        s["tag"] = [(j + m) % 16 | ((q[j] >> 1) & 1) << 4 | (1, 0, 1, 2)[q[j] % 4] << 5 for j in range(READS)]
        singles.append(s)
    assert set(state) == {0, 1, 2, 3, 4} and set(pairs["state"]) == {0, 1, 2} and any(p + L == N for p, L in zip(pos, lens))
    return types.SimpleNamespace(sym=sym, b=b, info=info, pairs=pairs, singles=singles)


@pytest.fixture(scope="module")
def matcher(case):
    import torch
    torch.zeros(1, device="cuda")      # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    m = UniqueMatcher(RealOptions(seedl=pw.SEEDL, seedkmax=pw.SEEDK, totalkmax=pw.TOTALK, scores=False, filter_level=pw.FILTER_LEVEL).normalise())
    m.set_text_symbols(FILEID, case.sym, np.array([0, N], dtype=np.uint64))
    yield m
    m.close()


def _three_stages(m, add, call_add, mismatches):
    """pileup, calls on the finished pileup, mismatch lists without singles -> their three statistics"""
    for reset in (m.pileup_stats, m.call_stats, m.mismatch_stats):
        reset(reset=True)
    m.pileup_begin(0)
    add()
    assert m.pileup_finish() > 0
    m.call_begin()
    call_add()
    m.call_finish(0, 0)
    got = mismatches()
    st = m.pileup_stats(), m.call_stats(), m.mismatch_stats()
    m.call_end()
    m.pileup_end()
    return st, got


def test_single_end_records_place_the_same_reads_in_all_three_stages(case, matcher):
    m, b = matcher, case.b
    want = pk.Pileup(case.sym, FILEID)
    want.add(b, case.info)
    # 10 hand-placed ends of the range: 2 end at n, 7 behind it (three of them with more than 32 bits), 1 of another file first
    assert want.stats["invalid"] == 7 and want.stats["other_file"] > 30 and want.stats["placed"] > 100, want.stats
    (pu, cl, mm), _ = _three_stages(m, lambda: m.pileup_add(b.bases, None, case.info, offsets=b.offsets),
                                    lambda: m.call_add(b.bases, None, case.info, offsets=b.offsets),
                                    lambda: m.mismatches(b.bases, None, case.info, offsets=b.offsets))
    for name, st in (("pileup", pu), ("calls", cl), ("mismatch lists", mm)):
        assert {k: st[k] for k in SHARED} == {k: want.stats[k] for k in SHARED} and st["reads"] == READS, (name, st, want.stats)
    assert pu["bases"] == mm["bases"] == want.stats["bases"]


def test_pair_records_place_the_same_mates_and_singles_add_exactly_the_checkers(case, matcher):
    m, b = matcher, case.b
    mate = (b.bases, None, b.offsets)
    want = pk.Pileup(case.sym, FILEID)
    want.add_pairs(b, b, case.pairs)
    assert want.stats["invalid"] > 5 and want.stats["other_file"] > 30 and want.stats["placed"] > 100, want.stats
    (pu, cl, mm), got = _three_stages(m, lambda: m.pileup_add_pairs(mate, mate, case.pairs), lambda: m.call_add_pairs(mate, mate, case.pairs),
                                      lambda: m.mismatches_pairs(mate, mate, case.pairs, cap=CAP))
    for name, st in (("pileup", pu), ("calls", cl), ("mismatch lists", mm)):
        assert {k: st[k] for k in SHARED} == {k: want.stats[k] for k in SHARED} and st["reads"] == 2 * READS, (name, st, want.stats)
    m.mismatch_stats(reset=True)
    reads = sk.pair_reads(b, b)
    without = sk.mismatch_lists(case.sym, FILEID, sk.final_pairs(case.pairs), reads)
    with_s = sk.mismatch_lists(case.sym, FILEID, sk.final_pairs(case.pairs, *case.singles), reads)
    assert {k: without[2][k] for k in SHARED} == {k: want.stats[k] for k in SHARED}
    # the singles of the NoMatch pairs alone: Unique ones of this file that fit are placed, the others counted as the pairs' are
    more = {k: with_s[2][k] - without[2][k] for k in SHARED}
    assert more["placed"] > 20 and more["other_file"] > 5 and more["invalid"] > 2, more
    for (gl, go), (wl, wo, wst), stats in ((got, without, mm), (m.mismatches_pairs(mate, mate, case.pairs, *case.singles, cap=CAP), with_s, None)):
        st = stats or m.mismatch_stats()
        assert np.array_equal(go, wo), np.nonzero(go != wo)[0][:10]
        assert all(np.array_equal(gl[k], wl[k]) for k in ("off", "ref", "base"))
        assert {k: st[k] for k in sk.COUNTERS} == wst, (st, wst)
    placed = lambda off: set(np.nonzero(off[1:] > off[:-1])[0].tolist())     # (every placed read has a substitution: its list is not empty)
    assert len(placed(with_s[1])) == with_s[2]["placed"] and placed(with_s[1]) - placed(without[1]) == \
        {j for j in range(2 * READS) if case.pairs["state"][j >> 1] == 0 and j in placed(with_s[1])}


def test_two_batch_calls_refuse_in_the_order_of_their_checks(case, matcher):
    """Two mates' batches that disagree are REAL_HIP_E_INVALID, but not before the checks that stand in front of that one:
    real_hip_mismatches_pairs has looked at its outputs by then (*n_out is 0, and null outputs are what it reports), and
    real_hip_pair_search on a context without a text answers REAL_HIP_E_STATE."""
    m, b = matcher, case.b
    full = m._read_batch(b.bases, None, b.offsets, host_records=True)
    half = m._read_batch(b.bases[:int(b.offsets[100])], None, b.offsets[:101], host_records=True)
    out, off, nout = np.zeros(64, dtype=rlib.MISMATCH_DTYPE), np.zeros(2 * READS + 1, dtype=np.uint64), C.c_uint64(77)
    two = m._L.real_hip_mismatches_pairs
    m.mismatch_stats(reset=True)
    args = (m._h, C.byref(full), C.byref(half), case.pairs.ctypes.data, None, None, out.ctypes.data, 64)
    assert two(*args, C.byref(nout), off.ctypes.data) == rlib.REAL_HIP_E_INVALID and nout.value == 0
    assert two(*args, C.byref(nout), None) == rlib.REAL_HIP_E_INVALID and "null mm_offsets" in m._L.real_hip_last_error(m._h).decode()
    assert m.mismatch_stats()["launches"] == 0
    bare = PairMatcher(m.opts)                                           # (no text)
    pp, sp = bare._pair_params(0, 500), bare._search_params(0)
    hits, hoff, rec = np.zeros(1, dtype=rlib.HIT_DTYPE), np.zeros(READS + 1, dtype=np.uint64), PairMatcher.new_pair_info(READS)
    lists = (hits.ctypes.data, hoff.ctypes.data, hits.ctypes.data, hoff.ctypes.data)
    search = lambda x: x._L.real_hip_pair_search(x._h, C.byref(pp), C.byref(sp), C.byref(full), C.byref(half), *lists, FILEID, 1, rec.ctypes.data)
    assert search(bare) == rlib.REAL_HIP_E_STATE
    bare.close()
    assert search(m) == rlib.REAL_HIP_E_INVALID                          # (with a text the disagreement is what is wrong)
