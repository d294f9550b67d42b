"""Mapping quality, the parts that need no GPU: the checker by hand, the header's tables against their formulas, the host-only
helpers real_hip_mapq_acc_merge / real_hip_mapq_of (the kernels' arithmetic, compiled from the same header) against the
checker, the ABI mirror, and the loud errors of `real -mapq / -pileup_minmapq`."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mapq_checker as mq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "real_amd", "host", "real")


# ---- the checker by hand ---------------------------------------------------------------------------------------------------
def test_checker_hand_cases():
    assert mq.quality(mq.acc_of_levels([7]), 7) == (60, False)                     # a lone candidate
    assert mq.quality(mq.acc_of_levels([7, 7]), 7) == (3, False)                   # two equal: 10 log10(2)
    assert mq.quality(mq.acc_of_levels([7, -5]), 7) == (18, False)                 # one candidate 12 levels (six bits) down
    assert mq.quality(mq.acc_of_levels([7, -5]), -5)[0] == 0                       # and the lower one's own quality
    assert mq.level_of_value(-0.25) == -1 and mq.level_of_value(-0.5) == -1 and mq.level_of_value(-0.75) == -2
    assert mq.level_of_value(0.49) == 0 and mq.level_of_value(3.5) == 7 and mq.level_of_value(-0.0) == 0
    assert mq.level_of_k(0) == 0 and mq.level_of_k(3) == -36
    # the window: 31 levels down is kept, 32 is dropped (and still counts in n)
    a = mq.acc_of_levels([0, -31, -32])
    assert (a["level"], a["n"], a["cnt"][31], sum(a["cnt"])) == (0, 3, 1, 2)
    # the top rises: what was inside falls out
    b = mq.merge(mq.acc_of_levels([-31, -30]), mq.acc_of_levels([1]))
    assert (b["level"], b["n"], b["cnt"][31], sum(b["cnt"])) == (1, 3, 1, 2)
    # saturation of a count at 255, of n at 2^32 - 1
    assert mq.acc_of_levels([4] * 255)["cnt"][0] == 255 and mq.acc_of_levels([4] * 256)["cnt"][0] == 255
    assert mq.acc_of_levels([4] * 256)["n"] == 256
    big = {"level": 4, "n": (1 << 32) - 2, "cnt": [255] + [0] * 31}
    assert mq.merge(big, mq.acc_of_levels([4]))["n"] == (1 << 32) - 1 and mq.merge(big, mq.acc_of_levels([4, 4]))["n"] == (1 << 32) - 1
    # unlisted: above the top, inside at an empty level, below the window, and against an empty accumulator
    acc = mq.acc_of_levels([10, 10, 8])
    assert mq.quality(acc, 12) == mq.quality(mq.acc_of_levels([12, 10, 10, 8]), 12)[:1] + (True,)
    assert mq.quality(acc, 9) == mq.quality(mq.acc_of_levels([10, 10, 9, 8]), 9)[:1] + (True,)
    assert mq.quality(acc, 10 - 32) == (0, True)
    assert mq.quality(mq.empty(), -40) == (60, True)
    assert mq.quality({"level": 99, "n": 0, "cnt": [9] * 32}, 5) == (60, True)       # n = 0 is empty whatever else it says
    # the second formulation agrees with the first
    rng = np.random.default_rng(5)
    for _ in range(300):
        lv = rng.integers(-50, 10, size=int(rng.integers(0, 400))) if rng.random() < 0.7 else rng.integers(-3, 1, size=int(rng.integers(0, 700)))
        assert mq.acc_of_levels(lv) == mq.sorted_acc_of_levels(lv)


def test_header_tables_against_the_formulas():
    hdr = open(os.path.join(ROOT, "include", "real_hip.h")).read()

    def table(name):
        body = re.search(r"#define\s+%s\s+\{(.*?)\}" % name, hdr, re.S).group(1)
        return [int(x) for x in re.findall(r"\d+", body.replace("\\", " "))]
    W, A = table("REAL_HIP_MAPQ_W_INIT"), table("REAL_HIP_MAPQ_A_INIT")
    assert len(W) == 32 and len(A) == 61
    assert W == mq.W and A == mq.A                                       # the checker's are exact integer roundings
    assert W == [round(2 ** 24 * 2 ** (-j / 2)) for j in range(32)]      # and the formulas as the header states them
    assert A == [round(16 * 10 ** (q / 10)) for q in range(61)]
    assert sum(255 * w for w in W) < 1 << 34 and sum(255 * w for w in W) * A[60] < 1 << 58
    for name, value in (("LEVELS", 32), ("MISMATCH_LEVELS", 12)):
        assert re.findall(r"#define\s+REAL_HIP_MAPQ_%s\s+(\d+)\b" % name, hdr) == [str(value)], name
    assert re.findall(r"#define\s+REAL_HIP_MAPQ_NONE\s+(\d+)u\b", hdr) == ["255"] and re.findall(r"#define\s+REAL_HIP_MAPQ_MAX\s+(\d+)u\b", hdr) == ["60"]
    assert re.findall(r"#define\s+REAL_HIP_ABI_VERSION\s+(\d+)", hdr) == ["2"]
    assert "REAL_HIP_K_COUNT = 8" in hdr


# ---- the host-only helpers ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rlib():
    from real_amd import lib
    lib.load()
    return lib


def _random_acc(rng):
    kind = rng.random()
    if kind < 0.08:
        return mq.empty()
    top = int(rng.integers(-2000, 2000)) if kind < 0.9 else int(rng.choice([-(1 << 31) + 1, (1 << 31) - 1, -(1 << 31) + 40, 0]))
    cnt = [int(c) for c in rng.choice([0, 0, 0, 1, 2, 7, 100, 128, 200, 254, 255], size=32)]
    cnt[0] = max(cnt[0], 1)                                              # the top level holds a candidate
    n = int(rng.choice([sum(cnt), sum(cnt) + 5, (1 << 32) - 1, (1 << 32) - 2, 1 << 31]))
    return {"level": top, "n": max(n, 1), "cnt": cnt}


def _merge_lib(rlib, a, b):
    return mq.acc_from_record(rlib.mapq_acc_merge(mq.acc_records([a])[0], mq.acc_records([b])[0]))


RISES = [0, 1, 7, 8, 9, 16, 24, 31, 32, 40]


def test_acc_merge_against_the_checker(rlib):
    rng = np.random.default_rng(11)
    for t in range(3000):
        a, b, c = _random_acc(rng), _random_acc(rng), _random_acc(rng)
        if t % 3 == 0 and a["n"] and a["level"] < (1 << 31) - 50:                 # the rises that cross each count word
            b["level"] = a["level"] + RISES[(t // 3) % len(RISES)]
        ab = _merge_lib(rlib, a, b)
        assert ab == mq.merge(a, b), (a, b)
        assert _merge_lib(rlib, b, a) == ab                                       # commutative, bit for bit
        assert _merge_lib(rlib, ab, c) == _merge_lib(rlib, a, _merge_lib(rlib, b, c)) == mq.merge(mq.merge(a, b), c)
    for d in RISES:                                                               # each rise by hand: one candidate d below a full window
        full = {"level": 5, "n": 32 * 255, "cnt": [255] * 32}
        got = _merge_lib(rlib, full, mq.acc_of_levels([5 + d]))
        assert got == mq.merge(full, mq.acc_of_levels([5 + d])) and got["level"] == 5 + d
        assert sum(got["cnt"]) == 255 * max(0, 32 - d) + (1 if d else 0) and got["cnt"][0] == (1 if d else 255)
    # an empty record is the neutral element, whatever its other fields say
    x = _random_acc(rng)
    assert _merge_lib(rlib, x, mq.empty()) == x == _merge_lib(rlib, {"level": 3, "n": 0, "cnt": [1] * 32}, x)
    assert _merge_lib(rlib, mq.empty(), mq.empty()) == mq.empty()
    L = rlib.load()
    one = mq.acc_records([x])
    assert L.real_hip_mapq_acc_merge(None, one.ctypes.data) == rlib.REAL_HIP_E_INVALID
    assert L.real_hip_mapq_acc_merge(one.ctypes.data, None) == rlib.REAL_HIP_E_INVALID


def test_mapq_of_against_the_checker(rlib):
    rng = np.random.default_rng(12)
    seen, unlisted = set(), 0
    for t in range(3000):
        a = _random_acc(rng)
        if abs(a["level"]) > 1 << 30:
            a["level"] = int(rng.integers(-100, 100))
        if t % 4 == 1:                                                   # few candidates
            a["cnt"] = [1] + [int(c) for c in rng.choice([0, 0, 0, 0, 0, 0, 1], size=31)]
        lp = a["level"] - int(rng.integers(-3, 36)) if a["n"] else int(rng.integers(-50, 50))
        if t % 4 == 3 and a["n"]:                                        # the best of two, the other j levels down: about 1.5 j, up to 46
            a["cnt"] = [1] + [0] * 31
            a["cnt"][1 + t // 4 % 31] = 1
            lp = a["level"]
        want = mq.quality(a, lp)
        assert rlib.mapq_of(mq.acc_records([a])[0], lp) == want, (a, lp)
        seen.add(want[0])
        unlisted += want[1]
    assert len(seen) >= 30 and max(seen - {60}) >= 45 and unlisted > 300 and {0, 3, 60} <= seen
    for levels, lp, want in (([7], 7, (60, False)), ([7, 7], 7, (3, False)), ([7, -5], 7, (18, False)), ([], 0, (60, True)),
                             ([10, 10, 8], 12, mq.quality(mq.acc_of_levels([10, 10, 8]), 12)), ([10], 10 - 32, (0, True))):
        assert rlib.mapq_of(mq.acc_records([mq.acc_of_levels(levels)])[0], lp) == want
    assert rlib.load().real_hip_mapq_of(None, 0, None) == rlib.REAL_HIP_E_INVALID
    assert rlib.load().real_hip_mapq_of(mq.acc_records([mq.empty()]).ctypes.data, 0, None) == 60        # unlisted is nullable


# ---- the library and the command line, without a device ---------------------------------------------------------------------
SYMBOLS = ["real_hip_mapq_acc_merge", "real_hip_mapq_of", "real_hip_mapq_hits", "real_hip_mapq_pair_hits", "real_hip_match_mapq",
           "real_hip_match_pairs_mapq", "real_hip_mapq", "real_hip_mapq_pairs", "real_hip_mapq_stats_get"]


def test_library_exports_the_mapping_quality(rlib):
    code = ("import sys; sys.path.insert(0, %r); from real_amd import lib; L = lib.load(); "
            "print([n for n in %r if not hasattr(L, n)], L.real_hip_abi_version())" % (ROOT, SYMBOLS))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stdout.decode().strip() == "[] 2", (r.stdout.decode(), r.stderr.decode()[-1000:])
    for name in SYMBOLS:
        assert name in rlib.ABI_SYMBOLS, name
    assert rlib.MAPQ_ACC_DTYPE == mq.ACC_DTYPE and rlib.MAPQ_ACC_DTYPE.itemsize == 40
    assert [rlib.MAPQ_ACC_DTYPE.fields[f][1] for f in ("level", "n", "cnt")] == [0, 4, 8]
    assert C.sizeof(rlib.RealHipMapqStats) == 8 + 7 * 8
    assert rlib.stats_fields(rlib.RealHipMapqStats) == ("folded", "candidates", "handed_over", "placements", "unlisted", "launches", "kernel_ms")
    assert (rlib.MAPQ_LEVELS, rlib.MAPQ_MISMATCH_LEVELS, rlib.MAPQ_MAX, rlib.MAPQ_NONE, rlib.MAPQ_EMPTY_LEVEL) == (
        mq.LEVELS, mq.MISMATCH_LEVELS, mq.MAX_Q, mq.NONE, mq.EMPTY_LEVEL)
    from real_amd.matcher import new_mapq_acc
    assert [mq.acc_from_record(r) for r in new_mapq_acc(3)] == [mq.empty()] * 3


def test_real_refuses_mapq_flags_that_cannot_work(tmp_path):
    """each before anything runs (no device is needed), non-zero, with a message of its own that names the flag"""
    fa, fq, fq2 = str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), str(tmp_path / "r2.fq")
    open(fa, "w").write(">g\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    for f in (fq, fq2):
        open(f, "w").write("@r\nACGTACGTACGTACGTACGTACGTACGTACGTAC\n+\n" + "I" * 34 + "\n")
    out, pf, vf, sf = str(tmp_path / "o.tsv"), str(tmp_path / "p.tsv"), str(tmp_path / "v.vcf"), str(tmp_path / "s.sam")
    base = [REAL, "-t", fa, "-p", fq, "-o", out]
    cases = [(base + ["-mapq", "1", "-u", "0"], b"-mapq 1 rates the unique placement of a read: it cannot be combined with -u 0"),
             (base + ["-p2", fq2, "-mapq", "1", "-pairs_all", "1"], b"-mapq 1 rates the unique placement of a fragment: it cannot be combined with -pairs_all 1"),
             (base + ["-pileup", pf, "-pileup_minmapq", "20"], b"-pileup_minmapq needs -mapq 1"),
             (base + ["-pileup", pf, "-mapq", "0", "-pileup_minmapq", "20"], b"-pileup_minmapq needs -mapq 1"),
             (base + ["-mapq", "1", "-pileup_minmapq", "20"], b"-pileup_minmapq is only meaningful with -pileup / -vcf"),
             (base + ["-mapq", "1", "-sam", sf, "-pileup_minmapq", "20"], b"-pileup_minmapq is only meaningful with -pileup / -vcf"),
             (base + ["-mapq", "1", "-pileup", pf, "-pileup_minmapq", "61"], b"-pileup_minmapq must be in 0..60"),
             (base + ["-mapq", "1", "-vcf", vf, "-pileup_minmapq", "-1"], b"-pileup_minmapq must be in 0..60")]
    for args, word in cases:
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode != 0 and word in r.stderr and b"unknown argument" not in r.stderr, (args, r.stderr.decode()[-600:])
        assert not any(os.path.exists(f) for f in (pf, vf, sf, out))
    r = subprocess.run([REAL, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    for word in (b"-mapq <0|1", b"-pileup_minmapq <Q"):
        assert word in r.stderr, word
