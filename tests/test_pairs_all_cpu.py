"""Every concordant pair of a fragment, without a GPU: the checker of the GPU tests against a second formulation and
against the existing per-fragment semantics (pairs_checker.check_pairs), the ABI mirror, and the -pairs_all flag through
the C++ parser (host_selftest) and the Python mirror."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from abi_header import header_structs
import pairs_all_checker as pac
import pairs_checker as pc
from real_amd import lib as rlib
from real_amd.matcher import RealOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT = np.dtype([("read", "<u4"), ("pos", "<u4"), ("score", "<f4"), ("frag", "<u2"), ("k", "u1"), ("inverted", "u1")])


def _random_lists(seed, n=100, most=12):
    """hand-made lists: clusters of hits around a few loci on two fragments and both strands, distinct inside a list"""
    rng = np.random.default_rng(seed)
    H, O, Ls = [[], []], [[0], [0]], [[], []]
    for i in range(n):
        locus = int(rng.integers(1000, 5000))
        for m in range(2):
            cnt = int(rng.integers(0, most + 1))
            seen = set()
            for _ in range(cnt):
                key = (int(locus + rng.integers(-60, 460)), int(rng.integers(0, 2)), int(rng.integers(0, 2)))
                if key in seen:
                    continue
                seen.add(key)
                H[m].append((i, key[0], float(-rng.integers(1, 12)) * 0.5, key[1], int(rng.integers(0, 4)), key[2]))
            O[m].append(len(H[m]))
            Ls[m].append(int(rng.integers(60, 121)))
    h = [np.array(x, dtype=HIT) if x else np.zeros(0, dtype=HIT) for x in H]
    return h[0], np.array(O[0], dtype=np.uint64), np.array(Ls[0], dtype=np.uint32), h[1], np.array(O[1], dtype=np.uint64), np.array(Ls[1], dtype=np.uint32)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_two_formulations_of_the_enumeration_agree(seed):
    L = _random_lists(seed)
    a, ao = pac.enumerate_pairs(*L, 150, 420, fileid=3)
    b, bo = pac.enumerate_pairs_flat(*L, 150, 420, fileid=3)
    assert a.shape[0] > 100 and np.array_equal(ao, bo)
    pac.assert_pair_hits_equal(b, a)
    per = (ao[1:] - ao[:-1]).astype(np.int64)
    assert (per == 0).any() and (per >= 2).any() and (a["inverted1"] == 0).any() and (a["inverted1"] == 1).any()
    assert (a["fileid"] == 3).all() and (a["reserved"] == 0).all() and (a["outer"] >= 150).all() and (a["outer"] <= 420).all()
    # row-major: inside a fragment the records follow the order of the product's cells
    h1, o1, _, h2, o2, _ = L
    for i in range(len(per)):
        A, B = h1[int(o1[i]):int(o1[i + 1])], h2[int(o2[i]):int(o2[i + 1])]
        ix = {(int(x["pos"]), int(x["frag"]), int(x["inverted"])): j for j, x in enumerate(A)}
        iy = {(int(y["pos"]), int(y["frag"]), int(y["inverted"])): j for j, y in enumerate(B)}
        cells = [ix[(int(r["pos1"]), int(r["frag"]), int(r["inverted1"]))] * len(B) + iy[(int(r["pos2"]), int(r["frag"]), 1 - int(r["inverted1"]))]
                 for r in a[int(ao[i]):int(ao[i + 1])]]
        assert cells == sorted(cells) and len(set(cells)) == len(cells)


@pytest.mark.parametrize("scores", [True, False])
def test_the_enumeration_reduces_to_the_per_fragment_records(scores):
    """the list, reduced under (value descending, location ascending), gives check_pairs' best, second and location"""
    L = _random_lists(7, n=80)
    h1, o1, l1, h2, o2, l2 = L
    recs, off = pac.enumerate_pairs(*L, 150, 420, fileid=2)
    want = pc.check_pairs([(2, h1, o1, h2, o2)], l1, l2, 150, 420, scores, 3 / 70.0)
    pac.assert_consistent_with_records(recs, off, want, scores)
    assert ((want["state"] != pc.NOMATCH) == ((off[1:] - off[:-1]) > 0)).all()
    assert (want["state"] == pc.NONUNIQUE).any() and (want["state"] == pc.UNIQUE).any()
    st = pac.expected_stats(o1, o2, recs)
    assert st["handed_over"] > 0 and st["products"] > st["pairs_out"] > 0


def test_pair_all_abi_mirror():
    assert C.sizeof(rlib.RealHipPairHit) == 32 and rlib.PAIR_HIT_DTYPE.itemsize == 32 and rlib.PAIR_HIT_DTYPE == pac.PAIR_HIT_DTYPE
    offsets = {"pair": 0, "pos1": 4, "pos2": 8, "outer": 12, "score1": 16, "score2": 20, "frag": 24, "fileid": 26, "inverted1": 27,
               "k1": 28, "k2": 29, "reserved": 30}
    for name, at in offsets.items():
        assert getattr(rlib.RealHipPairHit, name).offset == at and rlib.PAIR_HIT_DTYPE.fields[name][1] == at, name
    hdr = open(os.path.join(ROOT, "include", "real_hip.h")).read()
    names = header_structs()["real_hip_pair_hit"]
    assert names == list(rlib.PAIR_HIT_DTYPE.names), names
    assert C.sizeof(rlib.RealHipPairAllStats) == 56
    assert "#define REAL_HIP_ABI_VERSION 2" in hdr and re.search(r"REAL_HIP_K_COUNT = 8", hdr)


def test_pair_all_symbols_are_exported():
    L = rlib.load()
    for s in ("real_hip_pair_all_hits", "real_hip_match_pairs_all", "real_hip_pair_all_stats_get"):
        assert s in rlib.ABI_SYMBOLS and hasattr(L, s), s


def test_realoptions_pairs_all_flag(tmp_path):
    """-pairs_all through the C++ parser (host_selftest) and the Python mirror, and its loud errors"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "real_amd", "host"), "host_selftest"], stdout=subprocess.DEVNULL)
    st = os.path.join(ROOT, "real_amd", "host", "host_selftest")
    fq, fa = tmp_path / "m1.fq", tmp_path / "m2.fa"
    fq.write_text("@a\nACGT\n+\nIIII\n")
    fa.write_text(">a\nACGT\n")
    base = ["-t", "g.fa", "-p", str(fq), "-o", "out"]

    def run(cmd, args):
        return subprocess.run([st, cmd] + base + args, capture_output=True, text=True)
    for args, want in ((["-p2", str(fa), "-pairs_all", "1"], "1"), (["-p2", str(fa), "-pairs_all", "0"], "0"), (["-p2", str(fa)], "0"), ([], "0")):
        r = run("pairs_all_options", args)
        assert r.returncode == 0 and r.stdout.split() == [want], (args, r.stderr)
    for bad, word in ((["-pairs_all", "1"], "-pairs_all"), (["-pairs_all", "0"], "-pairs_all"),
                      (["-p2", str(fa), "-pairs_all", "1", "-mate_search", "1"], "-mate_search"),
                      (["-p2", str(fa), "-pairs_all", "1", "-u", "0"], "-u 0"), (["-p2", str(fa), "-u", "0"], "-u 0"),
                      (["-p2", str(fa), "-pairs_all"], "missing")):
        r = run("pairs_all_options", bad)
        assert r.returncode != 0 and word in r.stderr, (bad, r.stderr[-300:])
    assert run("pair_options", ["-p2", str(fa), "-pairs_all", "1", "-insert_min", "150", "-insert_max", "420"]).stdout.split() == \
        [str(fa), "0", "150", "420", "1"]                                          # pair_options keeps its output
    assert "-pairs_all" in subprocess.run([st, "options", "-h"], capture_output=True, text=True).stderr
    o = RealOptions.parse(base + ["-p2", "m2.fq", "-pairs_all", "1"])
    assert o.pairs_all and o.pattern2filename == "m2.fq"
    assert not RealOptions.parse(base + ["-p2", "m2.fq"]).pairs_all and not RealOptions.parse(base).pairs_all
    for bad, word in ((["-pairs_all", "1"], "-pairs_all"), (["-p2", "m2.fq", "-pairs_all", "1", "-mate_search", "1"], "-mate_search"),
                      (["-p2", "m2.fq", "-u", "0"], "-u 0"), (["-p2", "m2.fq", "-pairs_all", "1", "-u", "0"], "-u 0")):
        with pytest.raises(ValueError) as e:
            RealOptions.parse(base + bad)
        assert word in str(e.value), (bad, e.value)
