"""The pileup without a GPU: the checker (pileup_checker.py) on hand-made cases, what the shared workload
(pileup_workloads.py) must contain -- judged on the checker and the oracle's records alone -- and the parts of the library and
of the command line that need no device: the exported symbols, the site record's size, and the loud errors of `real`."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import pileup_checker as pk
import pileup_workloads as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "real_amd", "host", "real")


def _info(state, pos, fileid=0, frag=0, errors=0):
    return (state << 61) | (frag << 45) | (errors << 41) | (fileid << 35) | pos


def _batch(reads, quals=None):
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    return types.SimpleNamespace(bases=np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]),
                                 qual=None if quals is None else np.concatenate([np.asarray(q, dtype=np.uint8) for q in quals]), offsets=off)


#                 0  1  2  3  4  5  6  7  8  9
GENOME = np.array([0, 1, 2, 3, 4, 4, 3, 2, 1, 0], dtype=np.uint8)      # ACGTNNTGCA


def _pileup(reads, info, quals=None, min_qual=0, fileid=0):
    pu = pk.Pileup(GENOME, fileid, min_qual)
    pu.add(_batch(reads, quals), np.array(info, dtype=np.uint64))
    return pu


# ---- the checker, by hand -------------------------------------------------------------------------------------------
def test_checker_forward_read():
    pu = _pileup([[0, 1, 1, 3]], [_info(1, 0)])                        # ACCT over ACGT: C instead of G at 2
    assert pu.depth.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    s = pu.sites()
    assert s["pos"].tolist() == [2] and s["alt"].tolist() == [[0, 1, 0, 0]] and s["ref"].tolist() == [2] and s["depth"].tolist() == [1]
    assert pu.finish_stats() == dict(reads=1, placed=1, other_file=0, invalid=0, bases=4, mismatches=1, low_qual=0, n_dropped=0,
                                     covered=4, sites=1, max_depth=1)


def test_checker_reverse_read():
    # the read GCAT placed at 6 on the reverse strand shows its reverse complement ATGC over TGCA: A at 6 (T), T at 7 (G), G at 8 (C), C at 9 (A)
    pu = _pileup([[2, 1, 0, 3]], [_info(2, 6)])
    assert pu.depth.tolist() == [0] * 6 + [1] * 4
    s = pu.sites()
    assert s["pos"].tolist() == [6, 7, 8, 9] and s["alt"].tolist() == [[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0], [0, 1, 0, 0]]
    # and the read TGCA's reverse complement is TGCA itself: no site
    assert _pileup([[3, 2, 1, 0]], [_info(2, 6)]).sites().shape[0] == 0


def test_checker_quality_cut_follows_the_strand():
    reads, info = [[0, 1, 1, 0], [2, 1, 0, 3]], [_info(1, 0), _info(2, 6)]
    quals = [[40, 40, 19, 20], [5, 40, 40, 40]]                        # forward: base 2 has 19, base 3 has 20; reverse: text 9 <- read base 0 (quality 5)
    pu = _pileup(reads, info, quals, min_qual=20)
    assert pu.sites()["pos"].tolist() == [3, 6, 7, 8] and pu.stats["low_qual"] == 2 and pu.stats["mismatches"] == 4
    assert pu.depth.tolist() == [1, 1, 1, 1, 0, 0, 1, 1, 1, 1]          # the depth has no quality filter
    assert _pileup(reads, info, quals, min_qual=0).stats["mismatches"] == 6
    assert _pileup(reads, info, None, min_qual=30).stats["mismatches"] == 6 and _pileup(reads, info, None, min_qual=31).stats["mismatches"] == 0   # no qualities: 30


def test_checker_mismatch_on_an_n():
    pu = _pileup([[3, 1, 0, 0]], [_info(1, 3)])                         # T C A A over T N N T: C on an N, A on an N (stored as A: no mismatch), A over T
    assert pu.sites()["pos"].tolist() == [6] and pu.stats["n_dropped"] == 1 and pu.stats["mismatches"] == 1
    assert pu.depth[3:7].tolist() == [1, 1, 1, 1]


def test_checker_other_file_other_state_invalid():
    reads = [[0, 1, 1, 3]] * 5
    pu = _pileup(reads, [_info(1, 0, fileid=1), _info(4, 0), _info(0, 0), _info(3, 0), _info(1, 7)])
    assert pu.depth.sum() == 0 and pu.sites().shape[0] == 0
    st = pu.finish_stats()
    assert st["reads"] == 5 and st["other_file"] == 1 and st["invalid"] == 1 and st["placed"] == 0 and st["max_depth"] == 0
    assert _pileup(reads, [_info(1, 6)] * 5).finish_stats()["max_depth"] == 5     # ending exactly at n


def test_checker_pair():
    rec = np.zeros(3, dtype=pk.np.dtype([("pos1", "<u4"), ("pos2", "<u4"), ("fileid", "u1"), ("inverted1", "u1"), ("state", "u1")]))
    rec["state"] = [1, 2, 1]
    rec["pos1"], rec["pos2"], rec["inverted1"] = [0, 0, 6], [6, 6, 1], [0, 0, 1]
    b1 = _batch([[0, 1, 1, 3], [0, 0, 0, 0], [2, 1, 0, 3]])             # pair 0: ACCT forward at 0; pair 2: GCAT reverse at 6
    b2 = _batch([[2, 1, 0, 3], [0, 0, 0, 0], [1, 1, 2]])                # pair 0: GCAT reverse at 6; pair 2: CCG forward at 1 over CGT
    pu = pk.Pileup(GENOME)
    pu.add_pairs(b1, b2, rec)
    assert pu.depth.tolist() == [1, 2, 2, 2, 0, 0, 2, 2, 2, 2] and pu.stats["reads"] == 6 and pu.stats["placed"] == 4
    assert pu.sites()["pos"].tolist() == [2, 3, 6, 7, 8, 9] and pu.alt[2].tolist() == [0, 2, 0, 0] and pu.alt[6].tolist() == [2, 0, 0, 0]


# ---- what the workload must contain ---------------------------------------------------------------------------------
def test_workload_coverage(ora):
    w = pw.workload()
    info = pw.oracle_records(ora, "main", 1)[0]
    st, _, errors, _, pos = ora.unpack_record(info)
    placed = (st == 1) | (st == 2)
    lens = (w.main.offsets[1:] - w.main.offsets[:-1]).astype(np.int64)
    print("main: %d reads, %d placed (%d forward, %d reverse)" % (len(st), placed.sum(), (st == 1).sum(), (st == 2).sum()))
    assert placed.sum() > 1500 and (st == 1).sum() >= placed.sum() / 4 and (st == 2).sum() >= placed.sum() / 4
    assert set(((lens[placed] + 31) // 32).tolist()) == set(range(2, 11)) and lens.min() >= 33 and lens.max() == 320
    assert (pos[placed] == 0).any() and (pos[placed] + lens[placed] == w.g.n).any()
    assert (pos[placed] % 32 == 0).any() and (pos[placed] % 32 == 31).any()
    pu = pw.expected(ora, "main", 1, 0)
    s = pu.sites()
    assert ((s["alt"] > 0).sum(axis=1) >= 2).any() and (s["depth"] > 255).any() and pu.finish_stats()["max_depth"] >= 300
    assert int(errors[placed].sum()) == int(pu.alt.sum()) == pu.stats["mismatches"]      # min_qual 0: every counted error is an alt increment
    # (no matcher places a read over an N or behind the text: those two conditions are run on the device with hand-made
    # records, test_gpu_pileup.py)
    assert pu.stats["n_dropped"] == 0 and pu.stats["invalid"] == 0 and int(pu.depth.sum()) == pu.stats["bases"]
    cut = pw.expected(ora, "main", 1, 20)
    assert cut.stats["low_qual"] > 100 and cut.stats["low_qual"] + cut.stats["mismatches"] == pu.stats["mismatches"]
    assert (cut.depth == pu.depth).all()
    seen = 0
    for x, b in w.planted:
        if pu.depth[x]:
            seen += 1
            assert pu.alt[x].sum() > 0 and int(np.argmax(pu.alt[x])) == b, (x, b, pu.alt[x])
    assert seen >= 20
    lg = pw.oracle_records(ora, "long", 1)[0]
    ls = ora.unpack_record(lg)[0]
    ll = (w.long.offsets[1:] - w.long.offsets[:-1]).astype(np.int64)
    assert ((ls == 1) | (ls == 2)).sum() >= 30 and ll.min() == 321 and ll.max() == 700


# ---- the library and the command line, without a device -------------------------------------------------------------
SYMBOLS = ["real_hip_pileup_begin", "real_hip_pileup_add", "real_hip_pileup_add_pairs", "real_hip_pileup_finish", "real_hip_pileup_depth",
           "real_hip_pileup_sites", "real_hip_pileup_end", "real_hip_pileup_stats_get"]


def test_library_exports_the_pileup():
    from real_amd import lib as rlib
    L = rlib.load()
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert C.sizeof(rlib.RealHipPileupSite) == 32 and rlib.PILEUP_SITE_DTYPE.itemsize == 32 and pk.SITE_DTYPE == rlib.PILEUP_SITE_DTYPE
    assert C.sizeof(rlib.RealHipPileupParams) == 8 and C.sizeof(rlib.RealHipPileupStats) == 8 + 13 * 8
    assert L.real_hip_abi_version() == 2


def test_real_refuses_pileup_flags_that_cannot_work(tmp_path):
    """each before anything runs (no device is needed), non-zero, with a message of its own that names the flag"""
    fa, fq, fq2 = str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), str(tmp_path / "r2.fq")
    open(fa, "w").write(">g\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    for f in (fq, fq2):
        open(f, "w").write("@r\nACGTACGTACGTACGTACGTACGTACGTACGTAC\n+\n" + "I" * 34 + "\n")
    out, pf, df = str(tmp_path / "o.tsv"), str(tmp_path / "p.tsv"), str(tmp_path / "d.tsv")
    base = [REAL, "-t", fa, "-p", fq, "-o", out]
    cases = [(base + ["-pileup", pf, "-u", "0"], b"-pileup piles up the unique placements: it cannot be combined with -u 0"),
             (base + ["-pileup_depth", df, "-u", "0"], b"-pileup_depth piles up the unique placements: it cannot be combined with -u 0"),
             (base + ["-p2", fq2, "-pileup", pf, "-pairs_all", "1"], b"-pileup piles up the unique placement of a fragment: it cannot be combined with -pairs_all 1"),
             (base + ["-p2", fq2, "-pileup_depth", df, "-pairs_all", "1"], b"-pileup_depth piles up the unique placement of a fragment: it cannot be combined with -pairs_all 1"),
             (base + ["-pileup_minq", "20"], b"-pileup_minq is only meaningful with -pileup"),
             (base + ["-pileup_depth", df, "-pileup_minq", "20"], b"-pileup_minq is only meaningful with -pileup"),
             (base + ["-pileup", pf, "-pileup_minq", "64"], b"-pileup_minq takes a quality of at most 63"),
             (base + ["-pileup", out], b"same file as -o"), (base + ["-pileup", "-"], b"standard output (-) cannot be it"),
             (base + ["-pileup_depth", ""], b"need a file name"), (base + ["-pileup", pf, "-pileup_depth", pf], b"must name two files")]
    for args, word in cases:
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode != 0 and word in r.stderr and b"unknown argument" not in r.stderr, (args, r.stderr.decode()[-600:])
        assert not os.path.exists(pf) and not os.path.exists(df) and not os.path.exists(out)
    r = subprocess.run([REAL, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    for word in (b"-pileup <file", b"-pileup_depth <file", b"-pileup_minq <Q", b"-unpaired are NOT part of the pileup"):
        assert word in r.stderr, word
