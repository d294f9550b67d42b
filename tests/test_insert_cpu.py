"""Insert sizes, the parts that need no GPU: the checker against hand-computed cases, real_hip_insert_bounds (host only) against
the checker, what the bounds of a 200-fragment sample do on the whole-path workloads, the ABI mirror and the option rules of
-insert_hist / -insert_auto through the C++ parser and the Python mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from abi_header import header_structs
import insert_checker as ic
import insert_workloads as iw
import pairs_checker as pc
from real_amd import lib as rlib
from real_amd.matcher import PairMatcher, RealOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rec(rows):
    """rows of (pos1, pos2, inverted1, state)"""
    r = np.zeros(len(rows), dtype=pc.REC_DTYPE)
    for i, (p1, p2, inv, st) in enumerate(rows):
        r["pos1"][i], r["pos2"][i], r["inverted1"][i], r["state"][i] = p1, p2, inv, st
    return r


def test_checker_hand_cases():
    U, N, X = pc.UNIQUE, pc.NONUNIQUE, pc.NOMATCH
    rec = _rec([(100, 300, 0, U),        # mate 1 forward: 300 + 80 - 100 = 280
                (300, 100, 1, U),        # mate 2 forward: 300 + 100 - 100 = 300
                (100, 300, 0, N),        # not Unique
                (0, 0, 0, X),
                (500, 100, 0, U),        # forward behind reverse: invalid
                (100, 500, 1, U),        # the same with mate 2 forward: invalid
                (10, 10, 0, U),          # 10 + 80 - 10 = 80
                (0xfffffff0, 0xffffffff, 0, U),    # 2^32 - 1 + 80 - (2^32 - 16) = 95: needs 64 bits
                (7, 7, 1, U)])           # 7 + 100 - 7 = 100
    l1 = np.full(9, 100, dtype=np.uint32)
    l2 = np.full(9, 80, dtype=np.uint32)
    outer, valid = ic.outer_of(rec, l1, l2)
    assert [int(x) for x in outer[[0, 1, 6, 7, 8]]] == [280, 300, 80, 95, 100]
    assert [bool(v) for v in valid] == [True, True, True, True, False, False, True, True, True]
    h, st = ic.histogram(rec, l1, l2, 302)
    assert st == {"records": 9, "counted": 5, "overflow": 0, "invalid": 2}
    assert {int(d): int(h[d]) for d in np.nonzero(h)[0]} == {80: 1, 95: 1, 100: 1, 280: 1, 300: 1}
    h, st = ic.histogram(rec, l1, l2, 282)        # 280 is the last exact bin, 300 goes to the overflow bin 281
    assert (int(h[280]), int(h[281]), st["overflow"], st["counted"]) == (1, 1, 1, 5)
    h, st = ic.histogram(rec, l1, l2, 281)        # now both are in the overflow bin 280
    assert (int(h[280]), st["overflow"]) == (2, 2)
    h2, _ = ic.histogram(rec, l1, l2, 281, hist=h)
    assert (h2 == 2 * h).all()
    h, st = ic.histogram(rec, l1, l2, 2)
    assert [int(x) for x in h] == [0, 5] and st["overflow"] == 5
    # the quartile rule: 8 values 1 1 2 3 5 8 9 9 -> needs 2, 4, 6 -> q = 1, 3, 8
    hist = np.zeros(12, dtype=np.uint64)
    for v in (1, 1, 2, 3, 5, 8, 9, 9):
        hist[v] += 1
    assert ic.bounds(hist, 8) == (0, {"n": 8, "q1": 1, "median": 3, "q3": 8, "low": 0, "high": 29})
    assert ic.bounds(hist, 9)[0] == ic.E_STATE
    assert ic.bounds(hist, 8, 0) == (0, {"n": 8, "q1": 1, "median": 3, "q3": 8, "low": 1, "high": 8})
    # 5 values 10 10 10 10 11 in 13 bins: needs 2, 3, 4 -> all 10
    hist = np.zeros(13, dtype=np.uint64)
    hist[10], hist[11] = 4, 1
    assert ic.bounds(hist, 1) == (0, {"n": 5, "q1": 10, "median": 10, "q3": 10, "low": 10, "high": 10})
    hist[12] = 20                                # q3 in the overflow bin
    rc, est = ic.bounds(hist, 1)
    assert rc == ic.E_OVERFLOW and est["q3"] == 12


def _lib_bounds(hist, min_count, iqr_mult, n_bins=None):
    est = rlib.RealHipInsertEstimate()
    est.struct_size = C.sizeof(rlib.RealHipInsertEstimate)
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    rc = rlib.load().real_hip_insert_bounds(hist.ctypes.data, len(hist) if n_bins is None else n_bins, min_count, iqr_mult, C.byref(est))
    return rc, {"n": int(est.n), "q1": int(est.q1), "median": int(est.median), "q3": int(est.q3), "low": int(est.low), "high": int(est.high)}


def test_insert_bounds_against_the_checker():
    rng = np.random.default_rng(3)
    cases = []
    for _ in range(300):                          # random histograms: spread, concentrated, sparse, with and without overflow mass
        n_bins = int(rng.integers(2, 600))
        h = np.zeros(n_bins, dtype=np.uint64)
        k = int(rng.integers(0, 80))
        centre = int(rng.integers(0, n_bins))
        where = np.clip(rng.normal(centre, rng.integers(1, 60), size=k).astype(np.int64), 0, n_bins - 1)
        np.add.at(h, where, rng.integers(1, 1000, size=k).astype(np.uint64))
        cases.append((h, int(rng.integers(0, 40)), int(rng.integers(0, 5))))
    one = np.zeros(500, dtype=np.uint64)
    one[321] = 100000                             # all mass in one bin
    cases.append((one, 32, 3))
    for n in (31, 32, 33):                        # around REAL_HIP_INSERT_MIN_COUNT
        h = np.zeros(400, dtype=np.uint64)
        h[200:200 + n] = 1
        cases.append((h, rlib.REAL_HIP_INSERT_MIN_COUNT, 3))
    last = np.zeros(100, dtype=np.uint64)
    last[50], last[98] = 10, 30                   # q3 in the last exact bin
    cases.append((last, 32, 3))
    over = last.copy()
    over[98], over[99] = 0, 30                    # q3 in the overflow bin
    cases.append((over, 32, 3))
    low = np.zeros(1000, dtype=np.uint64)
    low[20], low[100] = 50, 50                    # q1 = 20 < 3 * 80: low saturates at 0
    cases.append((low, 32, 3))
    cases.append((np.array([40, 0], dtype=np.uint64), 32, 3))      # n_bins = 2, everything exact
    cases.append((np.array([10, 40], dtype=np.uint64), 32, 3))     # n_bins = 2, q3 in the overflow bin
    cases.append((np.array([0, 0], dtype=np.uint64), 0, 3))        # n = 0 has no quartiles, whatever min_count says
    big = np.zeros(16384, dtype=np.uint64)
    big[1], big[16000] = 1 << 40, 3 << 40         # counts beyond 32 bits
    cases.append((big, 32, 0xffffffff))           # high saturates at UINT32_MAX
    seen = set()
    for h, mc, mult in cases:
        want = ic.bounds(h, mc, mult)
        assert _lib_bounds(h, mc, mult) == want, (h, mc, mult)
        seen.add(want[0])
    assert seen == {0, ic.E_STATE, ic.E_OVERFLOW}
    assert _lib_bounds(one, 32, 3)[1] == {"n": 100000, "q1": 321, "median": 321, "q3": 321, "low": 321, "high": 321}
    assert [_lib_bounds(c[0], c[1], c[2])[0] for c in cases[301:304]] == [ic.E_STATE, 0, 0]
    assert _lib_bounds(last, 32, 3) == (0, {"n": 40, "q1": 50, "median": 98, "q3": 98, "low": 0, "high": 242})
    assert _lib_bounds(low, 32, 3)[1]["low"] == 0 and _lib_bounds(big, 32, 0xffffffff)[1]["high"] == 0xffffffff
    # bad arguments
    L = rlib.load()
    est = rlib.RealHipInsertEstimate()
    est.struct_size = C.sizeof(rlib.RealHipInsertEstimate)
    assert L.real_hip_insert_bounds(None, 10, 32, 3, C.byref(est)) == rlib.REAL_HIP_E_INVALID
    assert L.real_hip_insert_bounds(one.ctypes.data, 500, 32, 3, None) == rlib.REAL_HIP_E_INVALID
    assert _lib_bounds(one, 32, 3, n_bins=1)[0] == rlib.REAL_HIP_E_INVALID and _lib_bounds(one, 32, 3, n_bins=0)[0] == rlib.REAL_HIP_E_INVALID
    est.struct_size -= 4
    assert L.real_hip_insert_bounds(one.ctypes.data, 500, 32, 3, C.byref(est)) == rlib.REAL_HIP_E_INVALID
    # the Python wrapper
    assert PairMatcher.insert_bounds(one) == _lib_bounds(one, 32, 3)[1]
    for h, status in ((over, rlib.REAL_HIP_E_OVERFLOW), (cases[301][0], rlib.REAL_HIP_E_STATE)):
        with pytest.raises(rlib.RealHipError) as e:
            PairMatcher.insert_bounds(h)
        assert e.value.status == status


@pytest.mark.parametrize("kind,ragged", iw.WORKLOADS)
def test_bounds_of_a_sample_hold_the_library(ora, kind, ragged):
    """the bounds taken from the first 200 fragments under the window 0..1000 contain the outer distance of every Unique
    fragment of the workload, and the sample holds enough Unique fragments to take them from"""
    rec, l1, l2 = iw.records(ora, kind, ragged, 1)
    rc, est, (a, b) = iw.sample_bounds(rec[:iw.SAMPLE], l1[:iw.SAMPLE], l2[:iw.SAMPLE])
    outers = iw.unique_outers(rec, l1, l2)
    print(kind, ragged, "unique in the sample", est["n"], "of", iw.SAMPLE, "quartiles", est["q1"], est["median"], est["q3"], "bounds", (a, b),
          "outers", int(outers.min()), "..", int(outers.max()), "unique", len(outers))
    assert rc == 0 and est["n"] >= rlib.REAL_HIP_INSERT_MIN_COUNT
    assert est["n"] == int((rec["state"][:iw.SAMPLE] == pc.UNIQUE).sum())
    assert len(outers) > 1000 and a <= int(outers.min()) and int(outers.max()) <= b
    # a sample's records are those of the whole batch: a fragment's record does not depend on its neighbours
    rec_s, _, _ = iw.records(ora, kind, ragged, 1, n=iw.SAMPLE)
    pc.assert_records_equal(rec_s, rec[:iw.SAMPLE], "sample")


def test_insert_abi_mirror():
    hdr = open(os.path.join(ROOT, "include", "real_hip.h")).read()
    for name, cls, size in (("real_hip_insert_estimate", rlib.RealHipInsertEstimate, 40), ("real_hip_insert_stats", rlib.RealHipInsertStats, 56)):
        names = header_structs()[name]
        assert names == [n for n, _ in cls._fields_] and C.sizeof(cls) == size, names
    assert "#define REAL_HIP_INSERT_HIST_MAX_BINS %du" % rlib.REAL_HIP_INSERT_HIST_MAX_BINS in hdr and rlib.REAL_HIP_INSERT_HIST_MAX_BINS == ic.MAX_BINS
    assert "#define REAL_HIP_INSERT_MIN_COUNT %du" % rlib.REAL_HIP_INSERT_MIN_COUNT in hdr and rlib.REAL_HIP_INSERT_MIN_COUNT == ic.MIN_COUNT
    assert "#define REAL_HIP_ABI_VERSION 2" in hdr
    L = rlib.load()
    assert L.real_hip_abi_version() == 2
    for s in ("real_hip_pair_insert_hist", "real_hip_insert_bounds", "real_hip_insert_stats_get"):
        assert s in rlib.ABI_SYMBOLS and hasattr(L, s), s
    for name in ("insert_hist", "insert_bounds", "insert_stats"):
        assert hasattr(PairMatcher, name), name
    # the one formula: the kernel and the concordance test share it
    state = open(os.path.join(ROOT, "real_amd", "csrc", "pair_state.h")).read()
    kernel = open(os.path.join(ROOT, "real_amd", "csrc", "insert_hist.hip")).read()
    assert state.count("pair_outer(") == 2 and "pair_outer(" in kernel


def test_realoptions_insert_flags(tmp_path):
    """-insert_hist / -insert_auto through the C++ parser (host_selftest insert_options) and the Python mirror, and their loud errors"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "real_amd", "host"), "host_selftest"], stdout=subprocess.DEVNULL)
    st = os.path.join(ROOT, "real_amd", "host", "host_selftest")
    fq, fa = tmp_path / "m1.fq", tmp_path / "m2.fa"
    fq.write_text("@a\nACGT\n+\nIIII\n")
    fa.write_text(">a\nACGT\n")
    base = ["-t", "g.fa", "-p", str(fq), "-o", "out"]
    p2 = ["-p2", str(fa)]
    top = str(rlib.REAL_HIP_INSERT_HIST_MAX_BINS - 2)
    for args, want in ((p2, [".", "0", "0", "1000"]), (p2 + ["-insert_hist", "h.tsv"], ["h.tsv", "0", "0", "1000"]),
                       (p2 + ["-insert_auto", "5000", "-insert_min", "50", "-insert_max", "800"], [".", "5000", "50", "800"]),
                       (p2 + ["-insert_auto", "600", "-insert_hist", "h.tsv", "-insert_max", top, "-unpaired", "u.tsv"], ["h.tsv", "600", "0", top]),
                       (p2 + ["-insert_auto", "600", "-mate_search", "1"], [".", "600", "0", "1000"]),
                       (p2 + ["-insert_max", "20000"], [".", "0", "0", "20000"])):      # the limit holds with the two flags only
        r = subprocess.run([st, "insert_options"] + base + args, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.split() == want, (args, r.stderr)
    over = str(rlib.REAL_HIP_INSERT_HIST_MAX_BINS - 1)
    bad = ((["-insert_hist", "h.tsv"], "-p2"), (["-insert_auto", "600"], "-p2"),
           (p2 + ["-insert_hist", "h.tsv", "-pairs_all", "1"], "-pairs_all"), (p2 + ["-insert_auto", "600", "-pairs_all", "1"], "-pairs_all"),
           (p2 + ["-insert_hist", "h.tsv", "-insert_max", over], "-insert_max"), (p2 + ["-insert_auto", "600", "-insert_max", over], "-insert_max"),
           (p2 + ["-insert_hist", "out"], "-o"), (p2 + ["-insert_hist", "u.tsv", "-unpaired", "u.tsv"], "-unpaired"),
           (p2 + ["-unpaired", "u.tsv", "-insert_hist", "u.tsv"], "-unpaired"), (p2 + ["-insert_hist"], "missing"), (p2 + ["-insert_auto"], "missing"))
    for args, word in bad:
        r = subprocess.run([st, "insert_options"] + base + args, capture_output=True, text=True)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)
    help_text = subprocess.run([st, "options", "-h"], capture_output=True, text=True).stderr
    assert "-insert_hist" in help_text and "-insert_auto" in help_text and "FIRST genome file" in help_text
    o = RealOptions.parse(base + ["-p2", "m2.fq", "-insert_hist", "h.tsv", "-insert_auto", "600"])
    assert (o.inserthistfilename, o.insert_auto) == ("h.tsv", 600)
    assert (RealOptions.parse(base + ["-p2", "m2.fq"]).inserthistfilename, RealOptions.parse(base + ["-p2", "m2.fq"]).insert_auto) == ("", 0)
    for args, _ in bad:
        with pytest.raises(ValueError):
            RealOptions.parse(base + [("m2.fq" if a == str(fa) else a) for a in args])
