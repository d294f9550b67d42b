"""Duplicate marking without a device: the checker (dup_checker.py) on records written down by hand, the conditions of the
workloads the GPU tests rely on, the library's exports, and the flags `real` refuses."""
import ctypes as C
import os
import subprocess

import numpy as np

import dup_checker as dk
import dup_workloads as dw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "real_amd", "host", "real")


def test_checker_summaries():
    qual = np.array([0, 14, 15, 16, 63, 40, 2, 30], dtype=np.uint8)
    off = np.array([0, 3, 3, 8], dtype=np.uint64)
    s = dk.summaries(qual, off, 15)
    assert s["len"].tolist() == [3, 0, 5] and s["qsum"].tolist() == [15, 0, 16 + 63 + 40 + 30]
    assert dk.summaries(qual, off, 0)["qsum"].tolist() == [29, 0, 151]
    assert dk.summaries(qual, off, 63)["qsum"].tolist() == [0, 0, 63]
    assert dk.summaries(None, off, 30)["qsum"].tolist() == [90, 0, 150] and dk.summaries(None, off, 31)["qsum"].tolist() == [0, 0, 0]


def test_checker_single_end_by_hand():
    info, sums, want = dw.hand_single()
    keys = dk.keys_single(info, sums)
    assert keys[0] == (0, 1, 1000) and keys[1] == (0, 2, 1000) == keys[2] and keys[3] == (0, 2, 1010) and keys[4] == (1, 1, 1000)
    assert keys[6] is None and keys[7] is None and keys[14] is None
    assert keys[11] == keys[12] == (0, 2, (1 << 35) + 16382) and keys[13] != keys[12]
    dup, st, groups = dk.mark_single(info, sums)
    assert dup.tolist() == want.tolist()
    assert st == {"reads": 15, "placed": 12, "groups": 7, "duplicates": 5}
    assert groups[(0, 1, 1000)] == [0, 5, 8]


def test_checker_pairs_by_hand():
    pairs, s1, s2, want = dw.hand_pairs()
    keys = dk.keys_pairs(pairs, s1, s2)
    assert keys[0] == (0, 0, 100, 349) == keys[2] == keys[10] and keys[1] == (0, 1, 100, 349) and keys[3] == (0, 0, 100, 359)
    assert keys[5] == keys[6] == (0, 0, 5, (1 << 32) + 16382) and keys[7] == (0, 0, 5, 16382) and keys[8] is None and keys[9] is None
    dup, st, _ = dk.mark_pairs(pairs, s1, s2)
    assert dup.tolist() == want.tolist()
    assert st == {"reads": 11, "placed": 9, "groups": 6, "duplicates": 3}


def test_checker_line_and_masks():
    assert dk.stderr_line({"placed": 1926, "groups": 1622, "duplicates": 304}, 15) == "duplicates: placed=1926 groups=1622 duplicates=304 rate=0.1578 min_qual=15"
    assert dk.stderr_line({"placed": 0, "groups": 0, "duplicates": 0}, 0).endswith("rate=0.0000 min_qual=0")
    text = "@HD\tVN:1.6\nr1\t16\tg\t5\nr2\t0\tg\t9\nr3\t4\t*\t0\n"
    assert dk.sam_with_marks(text, {"r1"}) == "@HD\tVN:1.6\nr1\t1040\tg\t5\nr2\t0\tg\t9\nr3\t4\t*\t0\n"
    info, sums, want = dw.hand_single()
    masked = dk.masked_info(info, want)
    assert (masked[want != 0] == 0).all() and np.array_equal(masked[want == 0], info[want == 0])
    pairs, _, _, pdup = dw.hand_pairs()
    assert dk.masked_pairs(pairs, pdup)["state"].tolist() == [0, 1, 1, 1, 1, 1, 0, 1, 0, 2, 0]


def test_workload_conditions(ora):
    dw.assert_single_conditions(ora)
    dw.assert_pair_conditions(ora)
    rec, s1, s2, dup, st, groups = dw.pair_expected(ora)
    assert st == {"reads": 2382, "placed": 1917, "groups": 1805, "duplicates": 112}
    # the choice depends on min_qual: somewhere the representative changes with it
    _, _, dup15, _, _ = dw.single_expected(ora, "main")
    _, _, dup30, _, _ = dw.single_expected(ora, "main", min_qual=30)
    assert not np.array_equal(dup15, dup30) and dup15.sum() == dup30.sum()


def test_synthetic_records_have_groups_ties_and_unplaced():
    info, sums = dw.synthetic_records()
    dup, st, groups = dk.mark_single(info, sums)
    assert st["reads"] == 300_000 and st["placed"] < st["reads"] and st["duplicates"] > 50_000 and st["groups"] > 50_000
    assert max(len(m) for m in groups.values()) >= 8


def test_library_exports_the_duplicate_marking():
    from real_amd import lib as rlib
    L = rlib.load()
    for name in ("real_hip_read_summary", "real_hip_mark_duplicates", "real_hip_mark_duplicates_pairs", "real_hip_dup_stats_get"):
        assert hasattr(L, name) and name in rlib.ABI_SYMBOLS, name
    assert C.sizeof(rlib.RealHipReadSum) == 8 and rlib.READ_SUM_DTYPE.itemsize == 8 and rlib.READ_SUM_DTYPE == dk.SUM_DTYPE
    assert C.sizeof(rlib.RealHipDupStats) == 8 + 6 * 8
    assert rlib.DUP_STATS_FIELDS[:4] == dk.STATS
    assert L.real_hip_abi_version() == 2
    from real_amd.matcher import HipMatcher
    for name in ("read_summary", "mark_duplicates", "mark_duplicates_pairs", "dup_stats"):
        assert callable(getattr(HipMatcher, name))


def test_real_refuses_dedup_flags_that_cannot_work(tmp_path):
    """each before anything runs (no device is needed), non-zero, with a message of its own that names the flag"""
    fa, fq, fq2 = str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), str(tmp_path / "r2.fq")
    open(fa, "w").write(">g\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    for f in (fq, fq2):
        open(f, "w").write("@r\nACGTACGTACGTACGTACGTACGTACGTACGTAC\n+\n" + "I" * 34 + "\n")
    out = str(tmp_path / "o.tsv")
    base = [REAL, "-t", fa, "-p", fq, "-o", out]
    cases = [(base + ["-dedup", "1", "-u", "0"], b"-dedup marks copies of the unique placement of a read: it cannot be combined with -u 0"),
             (base + ["-p2", fq2, "-dedup", "1", "-pairs_all", "1"], b"-dedup marks copies of the unique placement of a fragment: it cannot be combined with -pairs_all 1"),
             (base + ["-dedup_minq", "10"], b"-dedup_minq needs -dedup 1"),
             (base + ["-dedup", "0", "-dedup_minq", "10"], b"-dedup_minq needs -dedup 1"),
             (base + ["-dedup", "1", "-dedup_minq", "64"], b"-dedup_minq must be in 0..63"),
             (base + ["-dedup", "1", "-dedup_minq", "-1"], b"-dedup_minq must be in 0..63"),
             (base + ["-dedup"], b"Parameter for argument -dedup is missing")]
    for args, word in cases:
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode != 0 and word in r.stderr and b"unknown argument" not in r.stderr, (args, r.stderr.decode()[-600:])
        assert not os.path.exists(out)
    r = subprocess.run([REAL, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    for word in (b"-dedup <0|1", b"-dedup_minq <n", b"FLAG 1024"):
        assert word in r.stderr, word
