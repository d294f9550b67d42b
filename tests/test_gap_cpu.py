"""Gap rescue, the parts that need no GPU: the checker's two formulations against each other, hand cases, real_hip_gap_cigar and the
struct sizes through ctypes, the loud errors that need no device, and the coverage floors of the workload the GPU tests run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from abi_header import header_structs
import gap_checker as gc
import gap_workloads as gw
from real_amd import lib as rlib
from real_amd.matcher import PairMatcher, RealOptions, new_gap_place

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MIN_PER_CLASS = 5


def _checked(ora, w, candidates=gc.cumsum_candidates):
    pairs, s1, s2, _ = gw.oracle_records(ora, w)
    t = gc.Text(w["g"].sym, w["g"].frag_start, w["fileid"])
    return gc.check_gap(t, w["b1"], w["b2"], pairs, s1, s2, w["min_ins"], w["max_ins"], w["prm"], candidates=candidates)


def test_the_two_formulations_agree_on_small_windows(ora):
    prm = gc.Params(3, 5, 4, 6, 1, 4 * 3 + 6 + 3, 0)
    w = gw.workload(seed=4, patl=30, prm=prm, n=40, min_ins=150, max_ins=215, frag_l=160, per_class=2)
    a, ca = _checked(ora, w)
    b, cb = _checked(ora, w, gc.brute_candidates)
    gc.assert_records_equal(a, b, "cumulative sums against explicit alignments")
    assert ca == cb and ca["placed"] >= 5 and ca["gapped"] >= 3, ca
    assert {int(x) for x in gc.state_of(a["tag"])} == {0, 1, 2}


def test_workload_meets_its_coverage_floors(ora):
    """asserted here, on the checker's records alone: no GPU test can pass by leaving a class out"""
    w = gw.workload()
    rec, ctr = _checked(ora, w)
    by_class, by_combo = gw.coverage(w, rec)
    print(ctr, by_class, by_combo)
    assert all(v >= MIN_PER_CLASS for v in by_class.values()), by_class
    assert all(v >= MIN_PER_CLASS for v in by_combo.values()), by_combo
    assert ctr["skipped"] > 0 and ctr["eligible"] > ctr["placed"] > ctr["unique"] > ctr["gapped"] > 0
    got = {j for p in w["plants"] if p["cls"] in "DI" for j in [p["split"]]}
    assert got >= {8, 31, 32, 33, 64, 92}, got
    assert {abs(p["g"]) for p in w["plants"] if p["cls"] in "DI"} == {1, 2, 7, 8}


def _text(seq, frag_start=None):
    sym = np.array(["ACGTN".index(c) for c in seq], dtype=np.uint8)
    return gc.Text(sym, frag_start or [0, len(seq)])


def _read(seq):
    return np.array(["ACGT".index(c) for c in seq], dtype=np.uint8)


RNG = np.random.default_rng(12)
BASE = "".join("ACGT"[x] for x in RNG.integers(0, 4, size=120))


def _both(t, r, first, last, prm, frag=0):
    fs, fe = t.frag_start[frag], t.frag_start[frag + 1]
    a = sorted(gc.cumsum_candidates(t, r, first, last, fs, fe, prm))
    b = sorted(gc.brute_candidates(t, r, first, last, fs, fe, prm))
    assert a == b
    return a


def test_hand_cases_cigar_and_leftmost_split():
    prm = gc.Params(3, 4, 4, 6, 1, 20, 0)
    t = _text(BASE)
    exact = _read(BASE[20:60])
    rec = gc.record_of(_both(t, exact, 15, 25, prm), prm, 0, 0, 0, 0)
    assert (int(rec["pos"]), int(rec["gap"]), int(rec["cost"]), gc.cigar_of(rec, 40)) == (20, 0, 0, "40M")
    dele = _read(BASE[20:38] + BASE[40:62])                              # two text bases gone behind 18 read bases
    rec = gc.record_of(_both(t, dele, 15, 25, prm), prm, 0, 0, 0, 0)
    assert (int(rec["pos"]), int(rec["gap"]), int(rec["k"]), int(rec["cost"])) == (20, 2, 0, 8) and gc.cigar_of(rec, 40).endswith("M2D%dM" % (40 - int(rec["split"])))
    assert int(rec["split"]) <= 18
    # a homopolymer: AAAA in the text, one A less in the read -- every split inside the run costs the same, the run's start wins
    hp = BASE[:30] + "G" + "AAAA" + "T" + BASE[36:80]
    t2 = _text(hp)
    r2 = _read(hp[10:31] + "AAA" + hp[35:51])
    rec = gc.record_of(_both(t2, r2, 8, 12, prm), prm, 0, 0, 1, 1)
    assert (int(rec["pos"]), int(rec["gap"]), int(rec["split"]), gc.cigar_of(rec, len(r2))) == (10, 1, 21, "21M1D19M")
    r3 = _read(hp[10:31] + "AAAAA" + hp[35:49])                          # one A more: an insertion, again at the run's start
    rec = gc.record_of(_both(t2, r3, 8, 12, prm), prm, 0, 0, 1, 1)
    assert (int(rec["pos"]), int(rec["gap"]), int(rec["split"]), gc.cigar_of(rec, len(r3))) == (10, -1, 21, "21M1I18M")
    assert int(gc.target_of(rec["tag"])) == 1 and int(gc.inverted_of(rec["tag"])) == 1 and int(gc.state_of(rec["tag"])) == gc.UNIQUE


def test_hand_cases_tie_order_and_second():
    prm = gc.Params(4, 4, 4, 6, 1, 30, 0)
    # (cost, |g|, p, g, j, k): equal costs -- ungapped first, then the shorter gap, the leftmost start, insertion before deletion, the leftmost split
    rows = [(8, 2, 50, 2, 9, 0), (8, 2, 50, -2, 9, 0), (8, 2, 50, -2, 7, 0), (8, 1, 51, 1, 9, 0), (8, 1, 50, 1, 30, 0), (8, 0, 60, 0, 0, 2)]
    order = []
    while rows:
        rec = gc.record_of(rows, prm, 0, 0, 0, 0)
        order.append((int(rec["gap"]), int(rec["pos"]), int(rec["split"])))
        rows = [r for r in rows if (r[3], r[2], r[4]) != order[-1]]
    assert order == [(0, 60, 0), (1, 50, 30), (1, 51, 9), (-2, 50, 7), (-2, 50, 9), (2, 50, 9)], order
    # a rival exactly max_gap starts away belongs to the same locus; one more and it votes
    best, near, far = (7, 1, 100, 1, 12, 0), (7, 1, 104, 1, 12, 0), (9, 1, 105, 1, 12, 0)
    rec = gc.record_of([best, near], prm, 0, 0, 0, 0)
    assert int(rec["second"]) == gc.NONE and int(gc.state_of(rec["tag"])) == gc.UNIQUE
    rec = gc.record_of([best, near, far], prm, 0, 0, 0, 0)
    assert int(rec["second"]) == 9 and int(gc.state_of(rec["tag"])) == gc.UNIQUE
    rec = gc.record_of([best, near, far], prm._replace(margin=2), 0, 0, 0, 0)
    assert int(gc.state_of(rec["tag"])) == gc.NONUNIQUE
    rec = gc.record_of([best, (7, 1, 95, 1, 12, 0)], prm, 0, 0, 0, 0)     # the best is the leftmost start, the other one a rival
    assert (int(rec["pos"]), int(rec["second"]), int(gc.state_of(rec["tag"]))) == (95, 7, gc.NONUNIQUE)


def test_hand_cases_max_cost_is_inclusive():
    t = _text(BASE)
    seq = list(BASE[20:60])
    for x in (3, 17, 29):
        seq[x] = "ACGT"[("ACGT".index(seq[x]) + 1) % 4]
    r = _read("".join(seq))
    at = gc.Params(2, 4, 4, 6, 1, 12, 0)
    assert [x[:4] for x in _both(t, r, 18, 22, at)] == [(12, 0, 20, 0)]
    assert _both(t, r, 18, 22, at._replace(max_cost=11)) == []
    dele = _read(BASE[20:38] + BASE[39:61])
    assert _both(t, dele, 18, 22, at._replace(max_cost=7))[0][:4] == (7, 1, 20, 1)
    assert _both(t, dele, 18, 22, at._replace(max_cost=6)) == []
    # an N inside the span, a span that leaves the fragment
    tn = _text(BASE[:45] + "N" + BASE[46:])
    assert _both(tn, _read(BASE[20:60]), 18, 22, at) == []
    assert _both(_text(BASE, [0, 59, 120]), _read(BASE[20:60]), 18, 22, at) == []


def test_abi_gap_structs_and_cigar():
    hs = header_structs()
    assert hs["real_hip_gap_place"] == list(rlib.GAP_PLACE_DTYPE.names) == list(gc.REC_DTYPE.names)
    assert hs["real_hip_gap_params"] == [f for f, _ in rlib.RealHipGapParams._fields_]
    assert hs["real_hip_gap_stats"][2:] == list(rlib.GAP_STATS_FIELDS)
    assert C.sizeof(rlib.RealHipGapPlace) == 16 and C.sizeof(rlib.RealHipGapParams) == 40 and C.sizeof(rlib.RealHipGapStats) == 88
    assert [rlib.GAP_PLACE_DTYPE.fields[f][1] for f in rlib.GAP_PLACE_DTYPE.names] == [gc.REC_DTYPE.fields[f][1] for f in gc.REC_DTYPE.names]
    rec = new_gap_place(3)
    assert rec.tobytes() == gc.empty_records(3).tobytes()
    rec["tag"] = gc.UNIQUE << 5
    rec["split"], rec["gap"] = [0, 40, 40], [0, 2, -3]
    for r, want in zip(rec, ("100M", "40M2D60M", "40M3I57M")):
        assert rlib.gap_cigar(r, 100) == want == gc.cigar_of(r, 100)
    L = rlib.load()
    buf = C.create_string_buffer(4)
    assert L.real_hip_gap_cigar(rec[1:].ctypes.data, 100, buf, 4) == rlib.REAL_HIP_E_OVERFLOW
    assert L.real_hip_gap_cigar(None, 100, buf, 4) == rlib.REAL_HIP_E_INVALID
    assert L.real_hip_gap_cigar(new_gap_place(1).ctypes.data, 100, buf, 4) == rlib.REAL_HIP_E_INVALID      # a NoMatch record has no CIGAR
    assert L.real_hip_gap_cigar(rec[2:].ctypes.data, 43, buf, 4) == rlib.REAL_HIP_E_INVALID                  # nothing aligned behind the insertion
    assert "real_hip_gap_rescue" in rlib.ABI_SYMBOLS and hasattr(L, "real_hip_gap_rescue") and hasattr(L, "real_hip_gap_stats_get")
    # without a context nothing runs
    assert L.real_hip_gap_rescue(None, None, None, None, None, None, None, None, 1, None) == rlib.REAL_HIP_E_INVALID
    assert L.real_hip_gap_stats_get(None, None, 0) == rlib.REAL_HIP_E_INVALID


def test_gap_params_defaults_follow_the_command_line():
    p = PairMatcher._gap_params(totalkmax=3)
    assert (p.max_gap, p.min_flank, p.cost_mismatch, p.cost_open, p.cost_extend, p.max_cost, p.margin) == (8, 8, 4, 6, 1, 26, 0)
    assert tuple(gc.default_params(3)) == (8, 8, 4, 6, 1, 26, 0)
    assert PairMatcher._gap_params(max_gap=16, totalkmax=5).max_cost == 42 and p.struct_size == 40


def test_realoptions_gapped_flags(tmp_path):
    """-gapped and -gap_* through the C++ parser (host_selftest gapped_options) and the Python mirror, and their loud errors"""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "real_amd", "host"), "host_selftest"], stdout=subprocess.DEVNULL)
    st = os.path.join(ROOT, "real_amd", "host", "host_selftest")
    fa = tmp_path / "m2.fa"
    fa.write_text(">r\nACGT\n")
    base = ["-t", "g.fa", "-p", str(fa), "-o", "out", "-e", "3"]

    def run(args):
        return subprocess.run([st, "gapped_options"] + base + args, capture_output=True, text=True)
    r = run(["-p2", str(fa), "-gapped", "g.tsv"])
    assert r.returncode == 0 and r.stdout.split() == ["g.tsv", "8", "8", "26", "0"], r.stderr
    r = run(["-p2", str(fa), "-gapped", "g.tsv", "-gap_max", "16", "-gap_flank", "5", "-gap_margin", "3", "-e", "5"])
    assert r.stdout.split() == ["g.tsv", "16", "5", "42", "3"], r.stderr
    assert run(["-p2", str(fa), "-gapped", "g.tsv", "-gap_maxcost", "30"]).stdout.split()[3] == "30"
    assert run(["-p2", str(fa)]).stdout.split()[0] == "."
    for bad, word in ((["-gapped", "g.tsv"], "-p2"), (["-p2", str(fa), "-gapped", "g.tsv", "-pairs_all", "1"], "-pairs_all"),
                      (["-p2", str(fa), "-gapped", "out"], "-o"), (["-p2", str(fa), "-gapped"], "missing"),
                      (["-p2", str(fa), "-gapped", "g.tsv", "-gap_max", "0"], "-gap_max"), (["-p2", str(fa), "-gapped", "g.tsv", "-gap_max", "17"], "-gap_max"),
                      (["-p2", str(fa), "-gapped", "g.tsv", "-gap_flank", "0"], "-gap_flank"), (["-p2", str(fa), "-gap_max", "4"], "-gapped"),
                      (["-p2", str(fa), "-gapped", "g.tsv", "-insert_max", "4097"], "-insert_max"),
                      (["-p2", str(fa), "-gapped", "g.tsv", "-sam", "g.tsv"], "same file")):
        r = run(bad)
        assert r.returncode == 1 and word in r.stderr, (bad, r.stderr)
    help_text = subprocess.run([st, "options", "-h"], capture_output=True, text=True).stderr
    assert all(f in help_text for f in ("-gapped", "-gap_max", "-gap_flank", "-gap_maxcost", "-gap_margin"))
    pybase = ["-t", "g.fa", "-p", "m1.fq", "-o", "out", "-e", "3"]
    o = RealOptions.parse(pybase + ["-p2", "m2.fq", "-gapped", "g.tsv"])
    assert (o.gappedfilename, o.gap_max, o.gap_flank, o.gap_maxcost, o.gap_margin) == ("g.tsv", 8, 8, 26, 0)
    assert RealOptions.parse(pybase + ["-p2", "m2.fq"]).gappedfilename == ""
    for bad in (["-gapped", "g.tsv"], ["-p2", "m2.fq", "-gapped", "g.tsv", "-pairs_all", "1"], ["-p2", "m2.fq", "-gapped", "out"],
                ["-p2", "m2.fq", "-gapped", "g.tsv", "-gap_max", "17"], ["-p2", "m2.fq", "-gapped", "g.tsv", "-insert_max", "4097"],
                ["-p2", "m2.fq", "-gapped"]):
        with pytest.raises(ValueError):
            RealOptions.parse(pybase + bad)
