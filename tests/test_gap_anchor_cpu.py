"""Anchored gap placement, the parts that need no GPU: the checker's two formulations of the union against each other, hand
cases for the four (e, v) diagonal rules, the merge M, the structs through ctypes, and the coverage floors of the workload the
GPU tests run -- on the checker's records over the CPU oracle's matchAll lists of S(b, A)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from abi_header import header_structs
import gap_anchor_checker as gac
import gap_anchor_workloads as gaw
import gap_checker as gc
from real_amd import lib as rlib
from real_amd.matcher import AllMatcher, RealOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIN_PER_CLASS = 5


def test_the_two_formulations_agree(ora):
    prm = gc.Params(3, 5, 4, 6, 1, 4 * 1 + 6 + 3, 0)
    w = gaw.workload(seed=4, patl=30, prm=prm, n=30, size=100_000, per_class=2)
    ap = gac.AnchorParams(12, 32)
    info, hits, hoff = gaw.oracle_lists(ora, w, ap.anchor_len)
    t = gc.Text(w["g"].sym, w["g"].frag_start, 0)
    a, ca = gac.check_anchor(t, w["b"], info, hits, hoff, prm, ap)
    b, cb = gac.check_anchor(t, w["b"], info, hits, hoff, prm, ap, candidates=gc.brute_candidates, union=gac.best_second_fold)
    gac.assert_records_equal(a, b, "flat set of cumulative sums against the per-anchor fold of explicit alignments")
    assert ca == cb and ca["placed"] >= 5 and ca["gapped"] >= 3 and ca["crowded"] >= 1, ca
    # folded into given records, both ways
    prev = a.copy()
    prev["fileid"] = 1
    c, _ = gac.check_anchor(t, w["b"], info, hits, hoff, prm, ap, out=prev)
    d, _ = gac.check_anchor(t, w["b"], info, hits, hoff, prm, ap, out=prev, union=gac.best_second_fold)
    gac.assert_records_equal(c, d, "folded")
    placed = gc.state_of(a["tag"]) != gc.NOMATCH
    assert (gc.state_of(c["tag"])[placed] == gc.NONUNIQUE).all() and (c["fileid"][placed] == 0).all()      # the same costs in two files


def test_workload_meets_its_coverage_floors(ora):
    """asserted here, on the checker's records alone: no GPU test can pass by leaving a class out"""
    w = gaw.workload()
    prm = w["prm"]
    ap = gac.AnchorParams(gaw.default_anchor(100, prm), 32)
    info, hits, hoff = gaw.oracle_lists(ora, w, ap.anchor_len)
    t = gc.Text(w["g"].sym, w["g"].frag_start, 0)
    rec, ctr = gac.check_anchor(t, w["b"], info, hits, hoff, prm, ap)
    by_class, by_strand = gaw.coverage(w, rec)
    print(ctr, by_class, by_strand)
    assert all(v >= MIN_PER_CLASS for v in by_class.values()), by_class
    assert all(v >= MIN_PER_CLASS for v in by_strand.values()), by_strand
    assert ctr["crowded"] >= MIN_PER_CLASS and ctr["skipped"] > 0 and ctr["reads"] > ctr["eligible"] > ctr["placed"] > ctr["unique"] > ctr["gapped"] > 0
    n_hits = np.diff(hoff.astype(np.int64))
    only = {c: sum(1 for p in w["plants"] if p["cls"] == c and gaw.intended(p, rec[p["i"]], w) and
                   n_hits[2 * p["i"] + (0 if (c == "P") == p["fwd"] else 1)] == 0) for c in "PS"}
    assert all(v >= MIN_PER_CLASS for v in only.values()), only                # one sub-read alone anchors these
    # a tail anchor whose diagonal lies in front of its fragment, and in front of the text
    fs = [int(x) for x in w["g"].frag_start]
    front = [p for p in w["plants"] if p["cls"] == "E" and p["g"] < 0 and p["xs"] in fs and gaw.intended(p, rec[p["i"]], w)]
    assert len(front) >= 2 and any(p["xs"] == 0 for p in front), front
    assert {p["split"] for p in w["plants"] if p["cls"] in "DI"} >= {8, 31, 32, 33, 64}
    assert {abs(p["g"]) for p in w["plants"] if p["cls"] in "DI"} == set(range(1, 9))


def _sym(seq):
    return np.array(["ACGTN".index(c) for c in seq], dtype=np.uint8)


RNG = np.random.default_rng(21)
BASE = "".join("ACGT"[x] for x in RNG.integers(0, 4, size=240))


class _B:
    def __init__(self, reads):
        self.bases = np.concatenate(reads)
        self.qual = None
        self.offsets = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)


def _hits(rows):
    h = np.zeros(len(rows), dtype=gac.HIT_DTYPE)
    for x, (read, pos, frag, inv) in enumerate(rows):
        h[x]["read"], h[x]["pos"], h[x]["frag"], h[x]["inverted"] = read, pos, frag, inv
    return h


def test_hand_cases_for_the_four_diagonal_rules():
    """R = text[50 .. 92) without its bases 70, 71: L = 40, a deletion of 2 behind 20 bases; A = 12.  R's head lies on diagonal
    50, its tail on diagonal 52: the tail's 12 bases start at text 52 + 28 = 80"""
    prm, ap, l = gc.Params(3, 4, 4, 6, 1, 20, 0), gac.AnchorParams(12, 4), 40
    t = gc.Text(_sym(BASE), [0, 240])
    r = _sym(BASE[50:70] + BASE[72:92])
    assert [gac.anchor_diagonal(q, e, v, l, 12) for q, e, v in ((50, 0, 0), (80, 1, 0), (80, 0, 1), (50, 1, 1))] == [50, 52, 52, 50]
    for v, read in ((0, r), (1, gc.COMP[r[::-1]])):
        for e, q in ((v, 50), (1 - v, 80)):                                    # the sub-read that is R's head, then its tail
            hoff = np.array([0, 1 - e, 1], dtype=np.uint64)
            rec, ctr = gac.check_anchor(t, _B([read]), None, _hits([(e, q, 0, v)]), hoff, prm, ap)
            assert (int(rec["pos"][0]), int(rec["gap"][0]), int(rec["k"][0]), int(rec["cost"][0]), int(rec["tag"][0])) == \
                (50, 2, 0, 8, (v << 4) | (gc.UNIQUE << 5)), (e, v, rec)
            assert int(rec["split"][0]) <= 20 and ctr["positions"] == 7 and ctr["anchors"] == 1
    # both anchors: overlapping windows count twice, the candidates once; the wrong strand finds nothing
    hoff = np.array([0, 1, 2], dtype=np.uint64)
    both, ctr = gac.check_anchor(t, _B([r]), None, _hits([(0, 50, 0, 0), (1, 80, 0, 0)]), hoff, prm, ap)
    assert (int(both["pos"][0]), int(both["gap"][0]), int(both["cost"][0])) == (50, 2, 8)
    assert ctr["positions"] == 14 and int(both["second"][0]) == gc.NONE
    none, ctr = gac.check_anchor(t, _B([r]), None, _hits([(0, 50, 0, 1)]), np.array([0, 1, 1], dtype=np.uint64), prm, ap)
    assert int(gc.state_of(none["tag"][0])) == gc.NOMATCH and ctr["placed"] == 0 and ctr["anchors"] == 1
    # invalid anchors: a fragment that is none, a sub-read that starts in front of its fragment or ends behind it
    t2 = gc.Text(_sym(BASE), [0, 45, 85, 240])
    bad = _hits([(0, 50, 3, 0), (0, 40, 1, 0), (1, 80, 1, 0)])
    rec, ctr = gac.check_anchor(t2, _B([r]), None, bad, np.array([0, 2, 3], dtype=np.uint64), prm, ap)
    assert ctr["invalid_anchors"] == 3 and ctr["anchors"] == 0 and ctr["positions"] == 0 and ctr["unanchored"] == 0
    # a diagonal in front of the text: R = text[0 .. 37) with 3 bases put in behind 20 -- the tail lies on diagonal -3
    ins = _sym(BASE[0:20] + "ACG" + BASE[20:37])
    rec, ctr = gac.check_anchor(t, _B([ins]), None, _hits([(1, 25, 0, 0)]), np.array([0, 0, 1], dtype=np.uint64), prm, ap)
    assert gac.anchor_diagonal(25, 1, 0, 40, 12) == -3 and ctr["positions"] == 1
    assert (int(rec["pos"][0]), int(rec["gap"][0]), int(rec["k"][0])) == (0, -3, 0) and "M3I" in gc.cigar_of(rec[0], 40)
    # the states that do not search: crowded, unanchored, skipped, not eligible
    many = _hits([(0, 50, 0, 0)] * 5)
    for hits, hoff, info, read, key in ((many, [0, 5, 5], None, r, "crowded"), (many[:0], [0, 0, 0], None, r, "unanchored"),
                                        (many[:1], [0, 1, 1], None, r[:10], "skipped"), (many[:1], [0, 1, 1], None, _sym("N" * 40), "skipped"),
                                        (many[:1], [0, 1, 1], np.array([1 << 61], dtype=np.uint64), r, None)):
        rec, ctr = gac.check_anchor(t, _B([read]), info, hits, np.array(hoff, dtype=np.uint64), prm, ap)
        assert rec.tobytes() == gc.empty_records(1).tobytes() and ctr["positions"] == 0
        assert (ctr[key] == 1 and ctr["eligible"] == 1) if key else ctr["eligible"] == 0


def _rec(pos, cost, second=gc.NONE, fileid=0, v=0, g=0, split=0, k=0, state=gc.UNIQUE):
    r = gc.empty_records(1)[0]
    r["pos"], r["cost"], r["second"], r["fileid"], r["gap"], r["split"], r["k"] = pos, cost, second, fileid, g, split, k
    r["tag"] = (v << 4) | (state << 5)
    return r


def test_merge_by_hand():
    G = 8
    empty = gc.empty_records(1)[0]
    a = _rec(100, 8, 12, g=2, split=30)
    for x, y in ((empty, a), (a, empty)):
        assert gac.merge(x, y, G, 0).tobytes() == a.tobytes(), "NoMatch is the neutral element"
    assert gac.merge(empty, empty, G, 0).tobytes() == empty.tobytes()
    # another locus of the same file: the loser's cost is a rival
    b = _rec(5000, 9)
    for x, y in ((a, b), (b, a)):
        m = gac.merge(x, y, G, 0)
        assert (int(m["pos"]), int(m["cost"]), int(m["second"]), int(gc.state_of(m["tag"]))) == (100, 8, 9, gc.UNIQUE)
        assert int(gc.state_of(gac.merge(x, y, G, 1)["tag"])) == gc.NONUNIQUE, "the state follows the call's margin"
    # the same start on the other strand is another locus; max_gap starts away on the same strand is the same one
    assert int(gac.merge(a, _rec(100, 9, v=1), G, 0)["second"]) == 9
    assert int(gac.merge(a, _rec(108, 9), G, 0)["second"]) == 12 and int(gac.merge(a, _rec(109, 9), G, 0)["second"]) == 9
    # ties: the ungapped one, then the shorter gap, the smaller file, the leftmost start, the forward strand, the insertion
    order = [_rec(300, 8, g=0, k=2, fileid=2), _rec(300, 8, g=1), _rec(200, 8, g=1, fileid=1), _rec(300, 8, g=-1, fileid=1),
             _rec(300, 8, g=1, fileid=1), _rec(300, 8, g=-1, fileid=1, v=1), _rec(300, 8, g=2, split=9), _rec(300, 8, g=2, split=10)]
    for x, y in itertools.combinations(range(len(order)), 2):
        m = gac.merge(order[y], order[x], 0, 0)
        assert gac.merge_key(m) == gac.merge_key(order[x]), (x, y)
    # across genome files M is commutative and associative: loci of different files are never the same
    rng = np.random.default_rng(3)
    for _ in range(200):
        recs = [_rec(int(rng.integers(90, 110)), int(rng.integers(4, 9)), int(rng.choice([gc.NONE, 6, 9, 12])), fileid=f, v=int(rng.integers(0, 2)),
                     g=int(rng.integers(-2, 3))) if rng.integers(0, 4) else empty for f in range(3)]
        ab_c = gac.merge(gac.merge(recs[0], recs[1], G, 2), recs[2], G, 2)
        a_bc = gac.merge(recs[0], gac.merge(recs[1], recs[2], G, 2), G, 2)
        ba_c = gac.merge(gac.merge(recs[1], recs[0], G, 2), recs[2], G, 2)
        c_ab = gac.merge(recs[2], gac.merge(recs[0], recs[1], G, 2), G, 2)
        assert ab_c.tobytes() == a_bc.tobytes() == ba_c.tobytes() == c_ab.tobytes()


def test_merge_is_conservative_across_blocks_of_one_file():
    """One file, three candidates: starts 92 (cost 6), 100 (cost 4) and 108 (cost 8), G = 8.  Examined in one call the best is
    100 and neither other start is more than G away: no rival, Unique.  Examined in two calls -- 100 alone, then 92 and 108 --
    the second call's best is 92 with second 8: 108 is 16 starts away from it.  Merged, the winner is 100 and the loser lies at
    its locus, but the loser's second still counts although 108 is within G of the winner"""
    G, prm = 8, gc.Params(8, 4, 4, 6, 1, 30, 3)
    rows = [(6, 0, 92, 0, 0, 0, 1, 0), (4, 0, 100, 0, 0, 0, 1, 0), (8, 0, 108, 0, 0, 0, 2, 0)]
    best, second = gac.best_second_flat([rows], prm)
    exact = gac.record_of(best, second, prm, 0)
    assert (int(exact["pos"]), int(exact["second"]), int(gc.state_of(exact["tag"]))) == (100, gc.NONE, gc.UNIQUE)
    one = gac.record_of(*gac.best_second_flat([rows[1:2]], prm), prm, 0)
    two = gac.record_of(*gac.best_second_flat([[rows[0], rows[2]]], prm), prm, 0)
    assert (int(two["pos"]), int(two["second"])) == (92, 8)
    for x, y in ((one, two), (two, one)):
        m = gac.merge(x, y, G, 3)
        assert (int(m["pos"]), int(m["cost"]), int(m["second"]), int(gc.state_of(m["tag"]))) == (100, 4, 8, gc.UNIQUE)
        assert int(gc.state_of(gac.merge(x, y, G, 4)["tag"])) == gc.NONUNIQUE          # exact: Unique whatever the margin
    # never wrongly Unique: M's second is at most the exact one
    assert int(m["second"]) <= int(exact["second"])


def test_abi_gap_anchor_structs():
    hs = header_structs()
    assert hs["real_hip_gap_anchor_params"] == [f for f, _ in rlib.RealHipGapAnchorParams._fields_]
    assert hs["real_hip_gap_anchor_stats"][2:] == list(rlib.GAP_ANCHOR_STATS_FIELDS) == list(gac.COUNTERS) + ["launches", "kernel_ms"]
    assert C.sizeof(rlib.RealHipGapAnchorParams) == 20 and C.sizeof(rlib.RealHipGapAnchorStats) == 8 + 13 * 8
    assert rlib.GAP_ANCHORS_MAX == gac.ANCHORS_MAX == 64
    assert [rlib.HIT_DTYPE.fields[f][1] for f in ("pos", "frag", "inverted")] == [gac.HIT_DTYPE.fields[f][1] for f in ("pos", "frag", "inverted")]
    p = AllMatcher._gap_anchor_params(46)
    assert (p.struct_size, p.anchor_len, p.max_anchors, p.reserved[0], p.reserved[1]) == (20, 46, 32, 0, 0)
    L = rlib.load()
    for name in ("real_hip_gap_anchor_hits", "real_hip_match_gapped", "real_hip_gap_anchor_stats_get"):
        assert name in rlib.ABI_SYMBOLS and hasattr(L, name)
    # without a context nothing runs
    assert L.real_hip_gap_anchor_hits(None, None, None, None, None, None, None, 1, None) == rlib.REAL_HIP_E_INVALID
    assert L.real_hip_match_gapped(None, None, None, None, None, 1, None) == rlib.REAL_HIP_E_INVALID
    assert L.real_hip_gap_anchor_stats_get(None, None, 0) == rlib.REAL_HIP_E_INVALID


def test_realoptions_gapped_single_flags(tmp_path):
    """-gapped_single, -gap_anchor and -gap_anchors through the C++ parser (host_selftest gapped_single_options) and the Python
    mirror, and their loud errors"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "real_amd", "host"), "host_selftest"], stdout=subprocess.DEVNULL)
    st = os.path.join(ROOT, "real_amd", "host", "host_selftest")
    fa = tmp_path / "m2.fa"
    fa.write_text(">r\nACGT\n")
    base = ["-t", "g.fa", "-p", str(fa), "-o", "out", "-e", "3"]

    def run(args):
        return subprocess.run([st, "gapped_single_options"] + base + args, capture_output=True, text=True)
    r = run(["-gapped_single", "g.tsv"])
    assert r.returncode == 0 and r.stdout.split() == ["g.tsv", "32", "32", "8", "8", "26", "0"], r.stderr
    r = run(["-gapped_single", "g.tsv", "-l", "48", "-gap_max", "16", "-gap_flank", "5", "-gap_margin", "3", "-e", "5", "-gap_anchors", "64"])
    assert r.stdout.split() == ["g.tsv", "48", "64", "16", "5", "42", "3"], r.stderr
    assert run(["-gapped_single", "g.tsv", "-gap_anchor", "46", "-gap_anchors", "1"]).stdout.split()[1:3] == ["46", "1"]
    assert run([]).stdout.split()[0] == "."
    for bad, word in ((["-p2", str(fa), "-gapped_single", "g.tsv"], "-gapped"), (["-gapped_single", "out"], "-o"), (["-gapped_single"], "missing"),
                      (["-gapped_single", "g.tsv", "-gap_anchor", "0"], "-gap_anchor"), (["-gapped_single", "g.tsv", "-gap_anchor", "321"], "-gap_anchor"),
                      (["-gapped_single", "g.tsv", "-gap_anchors", "0"], "-gap_anchors"), (["-gapped_single", "g.tsv", "-gap_anchors", "65"], "-gap_anchors"),
                      (["-gapped_single", "g.tsv", "-gap_max", "17"], "-gap_max"), (["-gapped_single", "g.tsv", "-u", "0"], "-u 0"),
                      (["-gap_anchor", "40"], "-gapped_single"), (["-gapped_single", "g.tsv", "-sam", "g.tsv"], "same file"),
                      (["-gapped", "g.tsv"], "-p2"), (["-gap_max", "4"], "-gapped")):
        r = run(bad)
        assert r.returncode == 1 and word in r.stderr, (bad, r.stderr)
    help_text = subprocess.run([st, "options", "-h"], capture_output=True, text=True).stderr
    assert all(f in help_text for f in ("-gapped_single", "-gap_anchor", "-gap_anchors"))
    pybase = ["-t", "g.fa", "-p", "m1.fq", "-o", "out", "-e", "3"]
    o = RealOptions.parse(pybase + ["-gapped_single", "g.tsv"])
    assert (o.gappedsinglefilename, o.gap_anchor, o.gap_anchors, o.gap_max, o.gap_flank, o.gap_maxcost, o.gap_margin) == ("g.tsv", 32, 32, 8, 8, 26, 0)
    assert RealOptions.parse(pybase).gappedsinglefilename == ""
    for bad in (["-p2", "m2.fq", "-gapped_single", "g.tsv"], ["-gapped_single", "out"], ["-gapped_single", "g.tsv", "-gap_anchor", "321"],
                ["-gapped_single", "g.tsv", "-gap_anchors", "65"], ["-gapped_single", "g.tsv", "-gap_max", "17"], ["-gapped", "g.tsv"]):
        with pytest.raises(ValueError):
            RealOptions.parse(pybase + bad)
