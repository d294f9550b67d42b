"""Paired-end reads on the device (real_hip_match_pairs / real_hip_pair_hits) against the brute-force checker of
pairs_checker.py, which works from the oracle's match_all lists and never calls the code under test."""
import ctypes as C

import numpy as np
import pytest

import pairs_checker as pc
import pairs_workloads as pw
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import PairMatcher, RealOptions, new_pair_info

pytestmark = pytest.mark.gpu

# scores, totalkmax, filter_level, table_kind, prefix_bits, seedl, ragged, (patl1, patl2)
CASES = [(1, 3, 2, 0, 0, 32, False, (100, 100)),
         (0, 3, 2, 3, 13, 16, False, (100, 80)),
         (0, 0, 2, 0, 0, 32, True, (100, 80)),
         (0, 3, 0, 2, 29, 32, False, (100, 80)),
         (1, 3, 2, 3, 13, 16, True, (100, 100))]
# scores on with epsilon = 0 (totalkmax 0, or filter level 0): the single-end fold never calls a tie NonUnique there
# (UpdateUniqueInfo compares with > on both sides), so no fragment can be "rescued" in the sense asserted above
ZERO_EPS_CASES = [(1, 0, 2, 0, 0, 32, True, (100, 80)), (1, 3, 0, 2, 29, 32, False, (100, 80))]


def _opts(seedl, totalkmax, scores, filter_level):
    return RealOptions(seedl=seedl, seedkmax=2, totalkmax=totalkmax, scores=bool(scores), filter_level=filter_level).normalise()


def _run_case(ora, kind, case, want_rescue):
    scores, tk, fl, tkind, pb, seedl, ragged, patl = case
    g, b1, b2 = pw.pair_workload(kind, ragged, patl)
    f, single = pw.oracle_pairs(ora, g, b1, b2, seedl, tk, scores, fl, want_single=True)
    want = pc.check_pairs([f], pw.lens_of(b1), pw.lens_of(b2), pw.MIN_INS, pw.MAX_INS, scores, ora.filter_mult(fl, tk))
    cov = pw.coverage(want, single)
    print(kind, case, cov)
    assert cov["nomatch"] and cov["unique"] and cov["nonunique"] and cov["fwd_first"] and cov["fwd_second"], cov
    if want_rescue:
        assert cov["rescued"] > 0, cov
    m = PairMatcher(_opts(seedl, tk, scores, fl), prefix_bits=pb, table_kind=tkind)
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    assert m.table_kind == {0: rlib.LAYOUT_STARTS, 2: rlib.LAYOUT_DIGEST, 3: rlib.LAYOUT_ROWS}[tkind], m.table_kind
    got = m.match_pairs(b1, b2, pw.MIN_INS, pw.MAX_INS)
    pc.assert_records_equal(got, want, "%s %r" % (kind, case))
    st = m.pair_stats()
    prod = ((f[2][1:] - f[2][:-1]).astype(np.int64) * (f[4][1:] - f[4][:-1]).astype(np.int64))
    assert st["pairs"] == b1.n_reads and st["products"] == int(prod.sum()), (st, int(prod.sum()))
    assert st["handed_over"] == int((prod > 32).sum()), (st, int((prod > 32).sum()))
    m.close()
    return st


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", ["iid", "families"])
def test_match_pairs_against_the_checker(ora, kind, case):
    st = _run_case(ora, kind, case, want_rescue=True)
    if kind == "families":
        assert st["handed_over"] > 0, "a 30- or 60-copy family gives products beyond a lane's budget"


@pytest.mark.parametrize("case", ZERO_EPS_CASES)
@pytest.mark.parametrize("kind", ["iid", "families"])
def test_match_pairs_scores_with_zero_epsilon(ora, kind, case):
    _run_case(ora, kind, case, want_rescue=False)


# ---- the join alone, on hand-made lists ---------------------------------------------------------------------------------
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


def _synthetic_fragments():
    F = []
    # 0: equal values at two locations: NonUnique, the smaller location is reported
    F.append(([(5000, 1, 0, 1, -3.0), (900, 1, 0, 1, -3.0)], [(5200, 1, 1, 0, -1.0), (1100, 1, 1, 0, -1.0)], 100, 100))
    # 1..4: outer distance exactly at the lower bound, one below, exactly at the upper bound, one above (bounds 150..420)
    F.append(([(1000, 0, 0, 0, -1.0)], [(1050, 0, 1, 0, -1.0)], 100, 100))    # 150
    F.append(([(1000, 0, 0, 0, -1.0)], [(1049, 0, 1, 0, -1.0)], 100, 100))    # 149
    F.append(([(1000, 0, 0, 0, -1.0)], [(1320, 0, 1, 0, -1.0)], 100, 100))    # 420
    F.append(([(1000, 0, 0, 0, -1.0)], [(1321, 0, 1, 0, -1.0)], 100, 100))    # 421
    # 5: the reverse mate ends in front of the forward mate's end (containment: f.pos + len_f > r.pos + len_r): rejected
    F.append(([(1000, 0, 0, 0, -1.0)], [(1010, 0, 1, 0, -1.0)], 200, 160))
    # 6: dovetail (the reverse mate starts in front of the forward one): rejected
    F.append(([(1000, 0, 0, 0, -1.0)], [(900, 0, 1, 0, -1.0)], 100, 300))
    # 7: different fragments; 8: same strand twice
    F.append(([(1000, 0, 0, 0, -1.0)], [(1200, 1, 1, 0, -1.0)], 100, 100))
    F.append(([(1000, 0, 0, 0, -1.0)], [(1200, 0, 0, 0, -1.0)], 100, 100))
    # 9: mate 2 is the forward one, with a clearly worse second placement: Unique
    F.append(([(2300, 2, 1, 2, -2.0), (7300, 2, 1, 3, -40.0)], [(2100, 2, 0, 0, -0.5), (7100, 2, 0, 1, -30.0)], 80, 120))
    # 10: no hits at all; 11: hits of one mate only
    F.append(([], [], 100, 100))
    F.append(([(10, 0, 0, 0, -1.0)] * 1, [], 100, 100))
    # 12: a large product (70 x 70): the wave path; one best, a runner-up far below, many non-concordant cells
    rng = np.random.default_rng(3)
    a = [(int(p), 3, 0, int(rng.integers(0, 4)), float(-rng.integers(5, 60))) for p in rng.permutation(70) * 1000 + 50_000]
    b = [(int(p), 3, 1, int(rng.integers(0, 4)), float(-rng.integers(5, 60))) for p in rng.permutation(70) * 1000 + 50_200]
    F.append((a, b, 100, 100))
    # 13: a large product with two equal best values (tie order inside the wave path)
    a = [(60_000 + 1000 * j, 4, 0, 1, -2.0) for j in range(40)]
    b = [(60_250 + 1000 * j, 4, 1, 1, -2.0) for j in range(40)]
    F.append((a, b, 100, 100))
    return F


def _checker_for_lists(L, scores, filter_mult, fileid=0):
    h1, o1, l1, h2, o2, l2 = L
    return pc.check_pairs([(fileid, h1, o1, h2, o2)], l1, l2, 150, 420, scores, filter_mult)


@pytest.mark.parametrize("scores", [1, 0])
def test_pair_hits_on_synthetic_lists(scores):
    F = _synthetic_fragments()
    m = PairMatcher(_opts(32, 3, scores, 2))
    L = _lists(F)
    want = _checker_for_lists(L, scores, m.opts.filter_mult)
    assert want["state"][0] == pc.NONUNIQUE and (want["pos1"][0], want["pos2"][0]) == (900, 1100)
    assert [int(s) for s in want["state"][1:9]] == [pc.UNIQUE, pc.NOMATCH, pc.UNIQUE, pc.NOMATCH] + [pc.NOMATCH] * 4
    assert want["state"][9] == pc.UNIQUE and want["inverted1"][9] == 1 and want["state"][13] == pc.NONUNIQUE
    m.pair_stats(reset=True)
    got = m.pair_hits(*L, 150, 420)
    pc.assert_records_equal(got, want, "host lists")
    st = m.pair_stats()
    assert st["pairs"] == len(F) and st["handed_over"] == 2 and st["products"] == sum(len(f[0]) * len(f[1]) for f in F), st
    # input order must not show: reversed and shuffled lists give the same records
    rng = np.random.default_rng(9)
    for perm in ("reversed", "shuffled"):
        G = []
        for a, b, la, lb in F:
            if perm == "reversed":
                G.append((a[::-1], b[::-1], la, lb))
            else:
                G.append(([a[j] for j in rng.permutation(len(a))], [b[j] for j in rng.permutation(len(b))], la, lb))
        pc.assert_records_equal(m.pair_hits(*_lists(G), 150, 420), want, perm)
    # device inputs: the same records
    import torch
    as_dev = {16: lambda x: x.view(np.int32).reshape(-1, 4), 8: lambda x: x.view(np.int64), 4: lambda x: x.view(np.int32)}
    dev = [torch.from_numpy(as_dev[x.dtype.itemsize](x).copy()).cuda() for x in L]
    rec = torch.zeros(len(F) * 40, dtype=torch.uint8, device="cuda")
    m.pair_hits(*dev, 150, 420, pairs=rec, fresh=True)
    pc.assert_records_equal(rec.cpu().numpy().view(rlib.PAIR_DTYPE), want, "device lists")
    m.close()


def test_pair_hits_folds_in_any_order_and_through_the_file_id():
    """the same lists as file 0 and as file 1: every pair exists twice, NonUnique through the file id alone; two different
    files folded in both orders give identical records"""
    F = _synthetic_fragments()
    m = PairMatcher(_opts(32, 3, 1, 2))
    L = _lists(F)
    h1, o1, l1, h2, o2, l2 = L
    rec = m.pair_hits(*L, 150, 420, fileid=0)
    rec = m.pair_hits(*L, 150, 420, fileid=1, pairs=rec)
    want = pc.check_pairs([(0, h1, o1, h2, o2), (1, h1, o1, h2, o2)], l1, l2, 150, 420, True, m.opts.filter_mult)
    pc.assert_records_equal(rec, want, "same lists as two files")
    had = _checker_for_lists(L, True, m.opts.filter_mult)["state"] != pc.NOMATCH
    assert had.any() and (rec["state"][had] == pc.NONUNIQUE).all() and (rec["fileid"][had] == 0).all()
    G = [(b_, a_, lb, la) for a_, b_, la, lb in F[::-1]] + F[:1]          # another file: other lists for the same number of fragments
    G = (G * 2)[:len(F)]
    G = [(a_, b_, F[i][2], F[i][3]) for i, (a_, b_, _, _) in enumerate(G)]
    L2 = _lists(G)
    ab = m.pair_hits(*L2, 150, 420, fileid=1, pairs=m.pair_hits(*L, 150, 420, fileid=0))
    ba = m.pair_hits(*L, 150, 420, fileid=0, pairs=m.pair_hits(*L2, 150, 420, fileid=1))
    pc.assert_records_equal(ab, ba, "fold order")
    want = pc.check_pairs([(0, h1, o1, h2, o2), (1, L2[0], L2[1], L2[3], L2[4])], l1, l2, 150, 420, True, m.opts.filter_mult)
    pc.assert_records_equal(ab, want, "two files")
    m.close()


@pytest.mark.parametrize("scores", [1, 0])
def test_two_genome_files_fold_in_both_orders(ora, scores):
    """two genome files and a stretch both hold (as test_two_genome_files_fold_through_the_file_id builds them): the
    records of match_pairs folded 0 then 1 and 1 then 0 are identical and equal the checker's over the union"""
    rng = np.random.default_rng(41)
    g0 = synth.random_genome(150_000, seed=501, n_frag=2)
    g1 = synth.random_genome(120_000, seed=502, n_frag=3)
    g1.sym[1000:2600] = g0.sym[1000:2600]                            # the same stretch at the same position (fragment 0 of both)
    assert g0.frag_start[1] > 2600 and g1.frag_start[1] > 2600
    pa = synth.sample_pairs(g0, 500, 100, 100, 300, 30, 0.01, 61, insert_min=150, insert_max=420)
    pb = synth.sample_pairs(g1, 400, 100, 100, 300, 30, 0.01, 62, insert_min=150, insert_max=420)
    shared = synth.Genome(sym=g0.sym[1000:2600].copy(), frag_start=np.array([0, 1600], dtype=np.uint64))
    ps = synth.sample_pairs(shared, 150, 100, 100, 300, 30, 0.0, 63, insert_min=150, insert_max=420, straddle_frac=0)
    b1 = synth.concat_batches([pa[0], pb[0], ps[0]])
    b2 = synth.concat_batches([pa[1], pb[1], ps[1]])
    files, recs = [], {}
    m = PairMatcher(_opts(32, 3, scores, 2))
    for order in ((0, 1), (1, 0)):
        rec = None
        for fid in order:
            g = (g0, g1)[fid]
            m.set_text_symbols(fid, g.sym, g.frag_start)
            m.build_index_block()
            rec = m.match_pairs(b1, b2, 150, 420, pairs=rec)
        recs[order] = rec
    for fid, g in enumerate((g0, g1)):
        files.append(pw.oracle_pairs(ora, g, b1, b2, 32, 3, scores, 2, fileid=fid)[0])
    want = pc.check_pairs(files, pw.lens_of(b1), pw.lens_of(b2), 150, 420, scores, m.opts.filter_mult)
    pc.assert_records_equal(recs[(0, 1)], want, "files 0, 1")
    pc.assert_records_equal(recs[(1, 0)], want, "files 1, 0")
    uniq = want["state"] == pc.UNIQUE
    assert (uniq & (want["fileid"] == 0)).sum() > 300 and (uniq & (want["fileid"] == 1)).sum() > 250
    assert (want["state"][-150:] == pc.NONUNIQUE).sum() >= 140, "pairs of the shared stretch are NonUnique through the file id"
    m.close()


def test_pair_errors_are_loud():
    g = synth.random_genome(50_000, seed=1)
    b1, b2 = synth.sample_pairs(g, 64, 100, 100, 300, 30, 0.0, 2)
    b3, _ = synth.sample_pairs(g, 63, 100, 100, 300, 30, 0.0, 2)
    m = PairMatcher(_opts(32, 3, 1, 2))
    with pytest.raises(rlib.RealHipError) as e:
        m.match_pairs(b1, b2, 150, 420)
    assert e.value.status == rlib.REAL_HIP_E_STATE            # no text / index yet
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    for args, kw, status in (((b1, b3, 150, 420), {}, rlib.REAL_HIP_E_INVALID),                     # unequal n_reads
                             ((b1, b2, 421, 420), {}, rlib.REAL_HIP_E_INVALID),                     # min > max
                             ((b1, b2, 150, 420), {"orientation": 1}, rlib.REAL_HIP_E_UNSUPPORTED)):
        with pytest.raises(rlib.RealHipError) as e:
            m.match_pairs(*args, **kw)
        assert e.value.status == status, (args[2:], kw, e.value)
    pp = PairMatcher._pair_params(150, 420)
    bb1, bb2 = m._mate_batch(b1), m._mate_batch(b2)
    assert m._L.real_hip_match_pairs(m._h, C.byref(bb1), C.byref(bb2), C.byref(pp), None) == rlib.REAL_HIP_E_INVALID   # null output
    assert m._L.real_hip_match_pairs(m._h, C.byref(bb1), C.byref(bb2), None, new_pair_info(64).ctypes.data) == rlib.REAL_HIP_E_INVALID
    L = _lists(_synthetic_fragments())
    ptr = [x.ctypes.data for x in L]
    assert m._L.real_hip_pair_hits(m._h, C.byref(pp), *ptr, len(L[2]), 0, 0, 1, None) == rlib.REAL_HIP_E_INVALID
    with pytest.raises(rlib.RealHipError) as e:
        m.pair_hits(*L, 421, 420)
    assert e.value.status == rlib.REAL_HIP_E_INVALID
    with pytest.raises(rlib.RealHipError) as e:
        m.pair_hits(*L, 150, 420, orientation=2)
    assert e.value.status == rlib.REAL_HIP_E_UNSUPPORTED
    # the context still works
    assert m.match_pairs(b1, b2, 150, 420).shape[0] == 64
    m.close()
