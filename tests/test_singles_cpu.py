"""Single placements of a mate, the parts that need no GPU: the checker against a second formulation on the whole-path
workloads, the fold's algebra, the ABI mirror, and the -unpaired flag through the C++ parser and the Python mirror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from abi_header import header_structs
import singles_checker as sc
import singles_workloads as sw
from real_amd import lib as rlib
from real_amd.matcher import PairMatcher, RealOptions, new_single_info

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", sw.CASES)
@pytest.mark.parametrize("kind", sw.KINDS)
def test_checker_agrees_with_a_second_formulation_on_the_workloads(ora, kind, case):
    w = sw.workload(ora, kind, case)
    print(kind, case, w["classes"], w["longer_than_32"])
    sw.assert_coverage(w, kind)
    scores = case[0]
    for m, (h, o, lens) in enumerate(((w["f"][1], w["f"][2], w["l1"]), (w["f"][3], w["f"][4], w["l2"]))):
        sc.assert_singles_equal(sc.sorted_singles([(0, h, o)], lens, scores, w["fm"]), w["s%d" % (m + 1)], "mate %d" % (m + 1))
    assert set(np.unique(sc.state_of(w["s1"]["tag"]))) == {0, 1, 2}


def _random_lists(rng, n, max_hits, scores):
    cnt = rng.integers(0, max_hits + 1, size=n)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    h = np.zeros(int(off[-1]), dtype=rlib.HIT_DTYPE)
    h["pos"] = rng.integers(0, 40, size=h.shape[0])
    h["frag"] = rng.integers(0, 2, size=h.shape[0])
    h["inverted"] = rng.integers(0, 2, size=h.shape[0])
    h["k"] = rng.integers(0, 3, size=h.shape[0])
    # (a location has one value wherever it appears: the score is a function of the location)
    h["score"] = -(((h["pos"] * 7 + h["frag"] * 3 + h["inverted"]) % 5).astype(np.float32) * np.float32(0.7)) if scores else 1.0
    if not scores:
        h["k"] = (h["pos"] + h["frag"] + h["inverted"]) % 3
    return h, off


def test_merge_of_the_files_is_the_record_of_the_union():
    rng = np.random.default_rng(5)
    for scores, fm in ((True, 3 / 70.0), (True, 0.0), (False, 3 / 70.0)):
        n = 400
        ha, oa = _random_lists(rng, n, 6, scores)
        hb, ob = _random_lists(rng, n, 3, scores)
        lens = rng.integers(20, 60, size=n).astype(np.uint32)
        files = [(0, ha, oa), (1, hb, ob)]
        want = sc.check_singles(files, lens, scores, fm)
        sc.assert_singles_equal(sc.sorted_singles(files, lens, scores, fm), want, "checker vs sorted")
        assert set(np.unique(sc.state_of(want["tag"]))) == {0, 1, 2}
        ra, rb = sc.check_singles(files[:1], lens, scores, fm), sc.check_singles(files[1:], lens, scores, fm)
        for x, y in ((ra, rb), (rb, ra)):
            m = np.array([sc.merge(x[i], y[i], scores, sc.eps_of(scores, fm, lens[i])) for i in range(n)], dtype=sc.REC_DTYPE)
            sc.assert_singles_equal(m, want, "merge of the files")
        # the same file twice: a location counts once
        m = np.array([sc.merge(ra[i], ra[i], scores, sc.eps_of(scores, fm, lens[i])) for i in range(n)], dtype=sc.REC_DTYPE)
        sc.assert_singles_equal(m, ra, "a file folded twice")


def test_merge_is_associative_and_commutative():
    rng = np.random.default_rng(6)
    pool = np.zeros(14, dtype=rlib.HIT_DTYPE)
    pool["pos"], pool["frag"], pool["inverted"] = rng.integers(0, 6, 14), rng.integers(0, 2, 14), rng.integers(0, 2, 14)
    pool["score"] = -((pool["pos"] * 7 + pool["frag"] * 3 + pool["inverted"]) % 4).astype(np.float32)
    for _ in range(400):
        sets = [pool[rng.choice(14, size=int(rng.integers(0, 4)), replace=False)] for _ in range(3)]
        fid = [int(x) for x in rng.integers(0, 2, 3)]
        a, b, c = (sc.record_of(sc.candidates(s, True, f), 0.5) for s, f in zip(sets, fid))
        ab_c = sc.merge(sc.merge(a, b, True, 0.5), c, True, 0.5)
        a_bc = sc.merge(a, sc.merge(b, c, True, 0.5), True, 0.5)
        assert ab_c.tobytes() == a_bc.tobytes()
        assert sc.merge(a, b, True, 0.5).tobytes() == sc.merge(b, a, True, 0.5).tobytes()
        union = sc.record_of(sum((sc.candidates(s, True, f) for s, f in zip(sets, fid)), []), 0.5)
        assert ab_c.tobytes() == union.tobytes()


def test_single_abi_mirror():
    hdr = open(os.path.join(ROOT, "include", "real_hip.h")).read()
    assert rlib.SINGLE_DTYPE.itemsize == 16 and rlib.SINGLE_DTYPE == sc.REC_DTYPE
    names = header_structs()["real_hip_single"]
    assert names == list(rlib.SINGLE_DTYPE.names), names
    names = header_structs()["real_hip_single_stats"]
    assert names == [n for n, _ in rlib.RealHipSingleStats._fields_] and C.sizeof(rlib.RealHipSingleStats) == 48, names
    for macro in ("REAL_HIP_SINGLE_K", "REAL_HIP_SINGLE_INVERTED", "REAL_HIP_SINGLE_STATE"):
        assert "#define %s(tag)" % macro in hdr
    tag = sc.make_tag(13, 1, 2)
    assert (int(rlib.single_k(tag)), int(rlib.single_inverted(tag)), int(rlib.single_state(tag))) == (13, 1, 2)
    assert "#define REAL_HIP_ABI_VERSION 2" in hdr and re.search(r"REAL_HIP_K_COUNT = 8 \}", hdr)
    L = rlib.load()
    assert L.real_hip_abi_version() == 2
    for s in ("real_hip_single_hits", "real_hip_match_pairs_singles", "real_hip_single_stats_get"):
        assert s in rlib.ABI_SYMBOLS and hasattr(L, s), s
    rec = new_single_info(3)
    assert (sc.state_of(rec["tag"]) == rlib.PAIR_NOMATCH).all() and np.isneginf(rec["second"]).all() and (rec["score"] == 0).all()
    assert rec.tobytes() == np.array([sc.empty_record()] * 3, dtype=sc.REC_DTYPE).tobytes()
    for name in ("single_hits", "match_pairs_singles", "single_stats", "new_single_info"):
        assert hasattr(PairMatcher, name), name


def test_realoptions_unpaired_flag(tmp_path):
    """-unpaired through the C++ parser (host_selftest unpaired_options) and the Python mirror, and its loud errors"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "real_amd", "host"), "host_selftest"], stdout=subprocess.DEVNULL)
    st = os.path.join(ROOT, "real_amd", "host", "host_selftest")
    fq, fa = tmp_path / "m1.fq", tmp_path / "m2.fa"
    fq.write_text("@a\nACGT\n+\nIIII\n")
    fa.write_text(">a\nACGT\n")
    base = ["-t", "g.fa", "-p", str(fq), "-o", "out"]
    r = subprocess.run([st, "unpaired_options"] + base + ["-p2", str(fa), "-unpaired", "u.tsv"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["u.tsv"], r.stderr
    r = subprocess.run([st, "unpaired_options"] + base + ["-p2", str(fa)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["."], r.stderr
    r = subprocess.run([st, "unpaired_options"] + base + ["-p2", str(fa), "-unpaired", "u.tsv", "-mate_search", "1"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["u.tsv"], r.stderr
    for bad, word in ((["-unpaired", "u.tsv"], "-p2"), (["-p2", str(fa), "-unpaired", "u.tsv", "-pairs_all", "1"], "-pairs_all"),
                      (["-p2", str(fa), "-unpaired", "out"], "-o"), (["-p2", str(fa), "-unpaired"], "missing")):
        r = subprocess.run([st, "unpaired_options"] + base + bad, capture_output=True, text=True)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr)
    assert "-unpaired" in subprocess.run([st, "options", "-h"], capture_output=True, text=True).stderr
    o = RealOptions.parse(base + ["-p2", "m2.fq", "-unpaired", "u.tsv"])
    assert (o.pattern2filename, o.unpairedfilename) == ("m2.fq", "u.tsv")
    assert RealOptions.parse(base + ["-p2", "m2.fq"]).unpairedfilename == ""
    for bad in (["-unpaired", "u.tsv"], ["-p2", "m2.fq", "-unpaired", "u.tsv", "-pairs_all", "1"], ["-p2", "m2.fq", "-unpaired", "out"],
                ["-p2", "m2.fq", "-unpaired"]):
        with pytest.raises(ValueError):
            RealOptions.parse(base + bad)
