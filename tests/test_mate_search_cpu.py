"""Mate search without a GPU: the checker (mate_search_checker.py) against a second, differently written formulation, the
workloads' coverage conditions, the ABI mirror of the new structs and the command-line flags with their loud errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from abi_header import header_structs
import mate_search_checker as mc
import mate_search_workloads as mw
import pairs_checker as pc
from real_amd import lib as rlib
from real_amd.matcher import RealOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("scores,totalkmax,filter_level,seedl,max_anchors", [(1, 3, 2, 32, 0), (0, 3, 0, 32, 0), (0, 5, 2, 16, 1)])
def test_checker_against_the_whole_genome_formulation(ora, scores, totalkmax, filter_level, seedl, max_anchors):
    g, b1, b2, _ = mw.search_workload("iid", False, (100, 80), seedl, totalkmax, n=64, size=120_000)
    f = mw.oracle_lists(ora, g, b1, b2, seedl, totalkmax, scores, filter_level)
    fm = ora.filter_mult(filter_level, totalkmax)
    args = (b1, b2, mw.MIN_INS, mw.MAX_INS, scores, fm, seedl, totalkmax)
    on, ctr = mc.check_pairs_search(ora, {0: g}, [f], *args, max_anchors=max_anchors)
    pc.assert_records_equal(on, mc.whole_genome_pairs(ora, g, 0, f, *args, max_anchors=max_anchors), "checker vs whole genome")
    off, _ = mc.check_pairs_search(ora, {0: g}, [f], *args, search=False)
    pc.assert_records_equal(off, pc.check_pairs([f], mw.lens_of(b1), mw.lens_of(b2), mw.MIN_INS, mw.MAX_INS, scores, fm), "search off")
    assert ctr["anchors"] > 0 and ctr["positions"] > ctr["anchors"] and ctr["placements"] > 0
    if max_anchors:
        assert ctr["anchors_skipped"] > 0, "the two-copy families give mates with two hits"
    else:
        mw.assert_coverage(off, on, f, "small genome")
    # the search alone and the join alone merge into the whole: the fold is the merge of two records
    alone, ctr2 = mc.search_only(ora, {0: g}, [f], *args, max_anchors=max_anchors)
    assert ctr2 == ctr
    merged = np.array([pc.merge(off[i], alone[i], pc.eps_of(scores, fm, *[int(mw.lens_of(b)[i]) for b in (b1, b2)])) for i in range(b1.n_reads)])
    pc.assert_records_equal(merged, on, "join merged with the search alone")


@pytest.mark.parametrize("kind,ragged,patl,seedl,totalkmax,scores,filter_level", [("iid", False, (100, 100), 32, 3, 1, 2),
                                                                                  ("families", True, (100, 80), 16, 5, 0, 0)])
def test_workloads_hold_every_state_change(ora, kind, ragged, patl, seedl, totalkmax, scores, filter_level):
    """the conditions of the GPU tests, met by the checker alone (the GPU tests assert them again for their own cases)"""
    g, b1, b2, planted = mw.search_workload(kind, ragged, patl, seedl, totalkmax)
    f = mw.oracle_lists(ora, g, b1, b2, seedl, totalkmax, scores, filter_level)
    args = (b1, b2, mw.MIN_INS, mw.MAX_INS, scores, ora.filter_mult(filter_level, totalkmax), seedl, totalkmax)
    off, _ = mc.check_pairs_search(ora, {0: g}, [f], *args, search=False)
    on, _ = mc.check_pairs_search(ora, {0: g}, [f], *args)
    tr = mw.assert_coverage(off, on, f, "%s %r" % (kind, patl))
    for cat, key in zip("ABCD", ("nomatch_unique", "nomatch_nonunique", "unique_nonunique", "unique_better")):
        assert set(planted[cat]) <= set(tr[key].tolist()), (cat, planted[cat], tr[key])
    same = (off["state"] == on["state"]) & (off["state"] != pc.NOMATCH)
    assert same.sum() > 100, "most fragments the seeds place stay as they are"


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("kind", ["iid", "families"])
@pytest.mark.parametrize("row", mw.PROTOCOL_ROWS, ids=[r.name for r in mw.PROTOCOL_ROWS])
def test_protocol_workloads_hold_every_state_change(ora, row, kind, scores):
    """the coverage conditions of test_gpu_pairs_protocols.py at every protocol shape, met by the checker alone"""
    g, b1, b2, planted = mw.protocol_search_workload(row, kind)
    f = mw.oracle_lists(ora, g, b1, b2, row.seedl, row.tk, scores, 2)
    args = (b1, b2, row.min_ins, row.max_ins, scores, ora.filter_mult(2, row.tk), row.seedl, row.tk)
    off, _ = mc.check_pairs_search(ora, {0: g}, [f], *args, search=False)
    on, _ = mc.check_pairs_search(ora, {0: g}, [f], *args)
    tr = mw.assert_coverage(off, on, f, "%s %s" % (row.name, kind))
    for cat, key in zip("ABCD", ("nomatch_unique", "nomatch_nonunique", "unique_nonunique", "unique_better")):
        assert set(planted[cat]) <= set(tr[key].tolist()), (cat, planted[cat], tr[key])
    lens = np.concatenate([mw.lens_of(b1), mw.lens_of(b2)])
    assert 550 <= b1.n_reads <= 650 and 300_000 <= g.n <= 400_000 and lens.max() == max(max(row.patl), max(max(p) for p in row.ragged_patl or [(0, 0)]))
    if kind == "families":
        n = b1.n_reads
        assert max(int(f[2][-1]), int(f[4][-1])) > n + n // 4 + 1024
    if row.ragged_patl:
        for b in (b1, b2):
            assert {(int(v) + 31) // 32 for v in mw.lens_of(b)} >= set(range(2, 11)), "every width in one batch"
        assert lens.min() == 36


def test_checker_against_the_whole_genome_formulation_at_150_bases(ora):
    """2 x 150 bases, 64-base seeds, five mismatches, inserts 200..700, random qualities: the checker against the second,
    differently written formulation on a small genome"""
    seedl, tk, scores, fl, mn, mx = 64, 5, 1, 2, 200, 700
    g, b1, b2, _ = mw.search_workload("iid", False, (150, 150), seedl, tk, n=40, size=200_000, min_ins=mn, max_ins=mx, frag_l=400, insert_mean=400,
                                      insert_sd=50, random_qual=True)
    f = mw.oracle_lists(ora, g, b1, b2, seedl, tk, scores, fl)
    fm = ora.filter_mult(fl, tk)
    args = (b1, b2, mn, mx, scores, fm, seedl, tk)
    on, ctr = mc.check_pairs_search(ora, {0: g}, [f], *args)
    pc.assert_records_equal(on, mc.whole_genome_pairs(ora, g, 0, f, *args), "checker vs whole genome")
    off, _ = mc.check_pairs_search(ora, {0: g}, [f], *args, search=False)
    mw.assert_coverage(off, on, f, "small genome, 150 bases")
    assert ctr["anchors"] > 0 and ctr["positions"] > ctr["anchors"] and ctr["placements"] > 0


def test_window_of_is_the_concordance_test():
    """every position: inside the window <=> concordant with the anchor and inside its fragment"""
    fs, fe = 1000, 3000
    for la, lb in ((100, 80), (80, 100), (100, 100)):
        for inv in (0, 1):
            for pa in (1000, 1200, 2000, 2900, fe - la):
                lo, hi = mc.window_of(pa, la, lb, inv, fs, fe, 150, 420)
                for p in range(fs - 50, fe + 50):
                    a = {"pos": pa, "frag": 0, "inverted": inv}
                    b = {"pos": p, "frag": 0, "inverted": 1 - inv}
                    want = pc.concordant(a, b, la, lb, 150, 420) and fs <= p and p + lb <= fe
                    assert (lo <= p <= hi) == want, (la, lb, inv, pa, p, lo, hi)


def test_mate_search_abi_mirror():
    hdr = open(os.path.join(ROOT, "include", "real_hip.h")).read()
    assert C.sizeof(rlib.RealHipMateSearchParams) == 16 and C.sizeof(rlib.RealHipMateSearchStats) == 64
    assert C.sizeof(rlib.RealHipPairParams) == 16 and C.sizeof(rlib.RealHipPairStats) == 32 and rlib.PAIR_DTYPE.itemsize == 40
    assert "#define REAL_HIP_ABI_VERSION 2" in hdr and re.search(r"REAL_HIP_K_COUNT = 8\b", hdr)
    for name, cls in (("real_hip_mate_search_params", rlib.RealHipMateSearchParams), ("real_hip_mate_search_stats", rlib.RealHipMateSearchStats)):
        names = header_structs()[name]
        assert names == [f for f, _ in cls._fields_], (name, names)
    assert int(re.search(r"#define REAL_HIP_MATE_SEARCH_MAX_INSERT (\d+)u", hdr).group(1)) == rlib.REAL_HIP_MATE_SEARCH_MAX_INSERT >= 2000
    new = ["real_hip_pair_search", "real_hip_match_pairs_search", "real_hip_mate_search_stats_get"]
    assert all(s in rlib.ABI_SYMBOLS for s in new)
    L = C.CDLL(rlib.LIB_PATH)
    for s in new:
        assert hasattr(L, s), s


def test_mate_search_flags(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "real_amd", "host"), "host_selftest"], stdout=subprocess.DEVNULL)
    st = os.path.join(ROOT, "real_amd", "host", "host_selftest")
    fq, fa = tmp_path / "m1.fq", tmp_path / "m2.fa"
    fq.write_text("@a\nACGT\n+\nIIII\n")
    fa.write_text(">a\nACGT\n")
    base = ["-t", "g.fa", "-p", str(fq), "-o", "out"]

    def run(extra):
        return subprocess.run([st, "mate_search_options"] + base + extra, capture_output=True, text=True)
    assert run(["-p2", str(fa)]).stdout.split() == ["0", "0"]                                   # off by default
    assert run([]).stdout.split() == ["0", "0"]
    assert run(["-p2", str(fa), "-mate_search", "1", "-mate_search_anchors", "50"]).stdout.split() == ["1", "50"]
    assert run(["-p2", str(fa), "-mate_search", "1", "-insert_max", str(rlib.REAL_HIP_MATE_SEARCH_MAX_INSERT)]).returncode == 0
    for bad, word in ((["-mate_search", "1"], "-p2"), (["-mate_search_anchors", "5"], "-p2"), (["-mate_search", "0"], "-p2"),
                      (["-p2", str(fa), "-mate_search", "1", "-insert_max", str(rlib.REAL_HIP_MATE_SEARCH_MAX_INSERT + 1)], "-insert_max"),
                      (["-p2", str(fa), "-mate_search"], "missing")):
        r = run(bad)
        assert r.returncode != 0 and word in r.stderr.split("Reads longer than")[-1], (bad, r.stderr[-300:])
    assert "-mate_search" in subprocess.run([st, "options", "-h"], capture_output=True, text=True).stderr
    o = RealOptions.parse(base + ["-p2", "m2.fq", "-mate_search", "1", "-mate_search_anchors", "9"])
    assert (o.mate_search, o.mate_search_anchors) == (True, 9)
    assert RealOptions.parse(base + ["-p2", "m2.fq"]).mate_search is False
    for bad in (["-mate_search", "1"], ["-mate_search_anchors", "3"],
                ["-p2", "m2.fq", "-mate_search", "1", "-insert_max", str(rlib.REAL_HIP_MATE_SEARCH_MAX_INSERT + 1)]):
        with pytest.raises(ValueError):
            RealOptions.parse(base + bad)
