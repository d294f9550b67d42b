"""Gapped mismatch lists, the parts that need no GPU: the checker's two formulations against each other on the records the gap
checker gives over the CPU oracle's lists and on the hand-made records, the coverage floors of what the GPU tests run, MD / NM by
hand, the round trip from a SAM line back to the text, the export and the header block, the flag's loud refusals and the C++
writer (host_selftest sam_gapped) against the checker's lines."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from abi_header import header_structs
import gap_checker as gc
import gap_workloads as gw
import gapped_list_checker as glc
import gapped_list_workloads as glw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "real_amd", "host", "host_selftest")
FLOOR = 5

_CACHE = {}


def _checked(ora):
    """the workload, its final records over the oracle's lists, and the gap checker's records: computed once"""
    if "w" not in _CACHE:
        w = glw.workload()
        pairs, s1, s2, _ = gw.oracle_records(ora, w)
        rec, _ = gc.check_gap(gc.Text(w["g"].sym, w["g"].frag_start, w["fileid"]), w["b1"], w["b2"], pairs, s1, s2, w["min_ins"], w["max_ins"], w["prm"])
        _CACHE["w"] = (w, pairs, s1, s2, rec)
    return _CACHE["w"]


def _assert_lists_equal(a, b, what):
    (la, oa, ca), (lb, ob, cb) = a, b
    assert np.array_equal(oa, ob), what
    assert la.tobytes() == lb.tobytes(), what
    assert ca == cb, (what, ca, cb)


def test_the_two_formulations_agree_on_the_workload_and_its_floors_hold(ora):
    w, _, _, _, rec = _checked(ora)
    a = glc.gapped_lists(w["g"].sym, 0, w["b1"], w["b2"], rec, glc.list_by_pairs)
    b = glc.gapped_lists(w["g"].sym, 0, w["b1"], w["b2"], rec, glc.list_by_diagonals)
    _assert_lists_equal(a, b, "aligned pairs against the diagonals' difference vectors")
    lists, off, ctr = a
    print(ctr)
    assert ctr["disagree"] == 0 and ctr["on_n"] == 0 and ctr["invalid"] == 0, ctr     # (the rescue admits no N in a span)
    uniq = gc.state_of(rec["tag"]) == gc.UNIQUE
    classes = {"deletion": uniq & (rec["gap"] > 0), "insertion": uniq & (rec["gap"] < 0), "ungapped with mismatches": uniq & (rec["gap"] == 0) & (rec["k"] > 0)}
    for name, sel in classes.items():
        assert int(sel.sum()) >= FLOOR, (name, int(sel.sum()))
        for tm in (0, 1):
            for inv in (0, 1):
                assert int((sel & (gc.target_of(rec["tag"]) == tm) & (gc.inverted_of(rec["tag"]) == inv)).sum()) >= 1, (name, tm, inv)
    # a first aligned mismatch directly behind the deleted bases: MD ...^AC0T...
    follows = 0
    for i in np.nonzero(classes["deletion"])[0]:
        L = lists[int(off[i]):int(off[i + 1])]
        g, j = int(rec["gap"][i]), int(rec["split"][i])
        follows += any(int(e["off"]) == j + g and int(e["base"]) != glc.DELETED for e in L)
    assert follows >= 1, follows


def test_the_two_formulations_agree_on_the_hand_made_records():
    h = glw.hand_cases()
    a = glc.gapped_lists(h["sym"], 0, h["b1"], h["b2"], h["gaps"], glc.list_by_pairs)
    b = glc.gapped_lists(h["sym"], 0, h["b1"], h["b2"], h["gaps"], glc.list_by_diagonals)
    _assert_lists_equal(a, b, "hand-made records")
    lists, off, ctr = a
    print(ctr)
    rec = h["gaps"]
    # what the hand-made set is for
    lens = np.array([int((h["b1"], h["b2"])[int(gc.target_of(r["tag"]))].offsets[i + 1] - (h["b1"], h["b2"])[int(gc.target_of(r["tag"]))].offsets[i])
                     for i, r in enumerate(rec)])
    n = h["sym"].shape[0]
    placed = np.array([gc.state_of(r["tag"]) == gc.UNIQUE and int(r["fileid"]) == 0 and glc.fits(r, int(l), n) for r, l in zip(rec, lens)])
    assert set(lens[placed]) == set(glw.LENGTHS) and set(rec["gap"][placed]) >= set(glw.GAPS)
    for l in glw.LENGTHS:
        for g in glw.GAPS:
            sel = placed & (lens == l) & (rec["gap"] == g)
            if g and l + min(g, 0) > 2:
                assert set(rec["split"][sel]) >= set(glw.splits_of(l, g)), (l, g)
    assert {(int(gc.target_of(t)), int(gc.inverted_of(t))) for t in rec["tag"][placed]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert (rec["pos"][placed] == 0).any() and (rec["pos"][placed].astype(np.int64) + lens[placed] + rec["gap"][placed] == n).any() and n % 32 and n % 64
    assert ctr["on_n"] > 0 and ctr["disagree"] > 0 and ((lists["ref"] == 4) & (lists["base"] == glc.DELETED)).any() and ((lists["ref"] == 4) & (lists["base"] < 4)).any()
    # the records that must give an empty list, and what counts them
    want = {"other_file": 0, "invalid": 0}
    for i, note in enumerate(h["what"]):
        if note in glw.EMPTY_NOTES:
            assert off[i + 1] == off[i], note
            if glw.EMPTY_NOTES[note]:
                want[glw.EMPTY_NOTES[note]] += 1
    assert (ctr["other_file"], ctr["invalid"]) == (want["other_file"], want["invalid"]) and want["invalid"] >= 11, ctr
    assert off[-1] > off[-2], "the fitting record behind the refused ones is listed"
    # an ungapped record's list is the ungapped checker's
    import sam_checker as sk
    for i in np.nonzero(placed & (rec["gap"] == 0))[0][:20]:
        r = rec[i]
        L = sk.placement_list(h["sym"], glc.target_read(h["b1"], h["b2"], r, i), int(r["pos"]), bool(gc.inverted_of(r["tag"])))
        assert L.tobytes() == lists[int(off[i]):int(off[i + 1])].tobytes()


def _list(rows):
    return glc._entries(rows)


@pytest.mark.parametrize("rows,span,g,md,nm", [
    ([], 100, 0, "100", 0),
    ([(40, 0, 4), (41, 1, 4)], 102, 2, "40^AC60", 2),
    ([(40, 0, 4), (41, 1, 4), (42, 3, 2)], 102, 2, "40^AC0T59", 3),
    ([(40, 3, 2)], 97, -3, "40T56", 4),                                   # an insertion behind 40 bases, the next aligned base differs: no trace of the insertion in MD
    ([(39, 2, 0)], 97, -3, "39G57", 4),                                   # ... the base in front of it
    ([(40, 0, 4), (41, 4, 4), (42, 2, 4)], 103, 3, "40^ANG60", 3),        # a deleted N of the text
    ([(0, 1, 2)], 100, 0, "0C99", 1),
    ([(99, 1, 2)], 100, 0, "99C0", 1),
    ([(0, 1, 2), (1, 4, 0), (50, 0, 4), (51, 2, 0), (101, 3, 0)], 102, 1, "0C0N48^A0G49T0", 5),
])
def test_md_and_nm_by_hand(rows, span, g, md, nm):
    L = _list(rows)
    assert glc.md_of(L, span) == md and glc.nm_of(L, g) == nm and glc.MD_RE.match(md)


def test_the_issue_example_with_57_behind_the_mismatch():
    assert glc.md_of(_list([(40, 0, 4), (41, 1, 4), (42, 3, 2)]), 100) == "40^AC0T57"


def test_reference_from_cigar_md_by_hand():
    assert glc.reference_from_cigar_md("ACGTACGT", "8M", "8") == "ACGTACGT"
    assert glc.reference_from_cigar_md("ACGTACGT", "4M2D4M", "4^TT4") == "ACGTTTACGT"
    assert glc.reference_from_cigar_md("ACGTACGT", "4M2D4M", "4^TT0C3") == "ACGTTTCCGT"
    assert glc.reference_from_cigar_md("ACGTGGACGT", "4M2I4M", "3A4") == "ACGAACGT"
    with pytest.raises(AssertionError):
        glc.reference_from_cigar_md("ACGT", "4M", "5")


def test_every_workload_record_rebuilds_the_text(ora):
    w, _, _, _, rec = _checked(ora)
    lists, off, _ = glc.gapped_lists(w["g"].sym, 0, w["b1"], w["b2"], rec)
    letters = "".join("ACGTN"[c] for c in w["g"].sym)
    seen = 0
    for i in np.nonzero(gc.state_of(rec["tag"]) == gc.UNIQUE)[0]:
        r = rec[i]
        read = gc.oriented(glc.target_read(w["b1"], w["b2"], r, i), bool(gc.inverted_of(r["tag"])))
        l, g, p = int(read.shape[0]), int(r["gap"]), int(r["pos"])
        L = lists[int(off[i]):int(off[i + 1])]
        seq = "".join("ACGT"[c] for c in read)
        assert glc.reference_from_cigar_md(seq, gc.cigar_of(r, l), glc.md_of(L, l + g)) == letters[p:p + l + g], i
        assert glc.nm_of(L, g) == int(r["k"]) + abs(g)
        seen += 1
    assert seen >= 60
    h = glw.hand_cases()
    lists, off, _ = glc.gapped_lists(h["sym"], 0, h["b1"], h["b2"], h["gaps"])
    letters = "".join("ACGTN"[c] for c in h["sym"])
    for i in np.nonzero(np.diff(off.astype(np.int64)) > 0)[0]:
        r = h["gaps"][i]
        read = gc.oriented(glc.target_read(h["b1"], h["b2"], r, i), bool(gc.inverted_of(r["tag"])))
        l, g, p = int(read.shape[0]), int(r["gap"]), int(r["pos"])
        seq = "".join("ACGT"[c] for c in read)
        assert glc.reference_from_cigar_md(seq, gc.cigar_of(r, l), glc.md_of(lists[int(off[i]):int(off[i + 1])], l + g)) == letters[p:p + l + g], h["what"][i]


def test_abi_export_header_block_and_mirror():
    from real_amd import lib as rlib
    from real_amd.matcher import PairMatcher
    header = open(os.path.join(ROOT, "include", "real_hip.h")).read()
    assert "#define REAL_HIP_ABI_VERSION 2" in header and "REAL_HIP_K_COUNT = 8" in header
    assert "#define REAL_HIP_MISMATCH_DELETED 4u" in header and "gapped mismatch lists" in header
    assert rlib.MISMATCH_DELETED == glc.DELETED == 4
    hs = header_structs()
    assert hs["real_hip_gapped_list_stats"][2:] == list(rlib.GAPPED_LIST_STATS_FIELDS)
    assert tuple(rlib.GAPPED_LIST_STATS_FIELDS[:-2]) == glc.COUNTERS
    assert C.sizeof(rlib.RealHipGappedListStats) == 8 + 12 * 8 and C.sizeof(rlib.RealHipMismatch) == 4
    assert C.sizeof(rlib.RealHipGapStats) == 88 and C.sizeof(rlib.RealHipMismatchStats) == 88 and C.sizeof(rlib.RealHipGapPlace) == 16   # no struct grew
    L = rlib.load()
    for name in ("real_hip_mismatches_gapped", "real_hip_gapped_list_stats_get"):
        assert name in rlib.ABI_SYMBOLS and hasattr(L, name)
    assert L.real_hip_mismatches_gapped(None, None, None, None, None, 0, None, None) == rlib.REAL_HIP_E_INVALID
    assert L.real_hip_gapped_list_stats_get(None, None, 0) == rlib.REAL_HIP_E_INVALID
    assert callable(PairMatcher.mismatches_gapped) and callable(PairMatcher.gapped_list_stats)
    mk = open(os.path.join(ROOT, "real_amd", "csrc", "Makefile")).read()
    assert "gapped_list.o" in mk


def _selftest_built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "real_amd", "host"), "host_selftest"], stdout=subprocess.DEVNULL)


def test_realoptions_sam_gapped_flag(tmp_path):
    """-sam_gapped through the C++ parser (host_selftest sam_gapped_options): what it needs, loudly"""
    _selftest_built()
    fa = tmp_path / "m2.fa"
    fa.write_text(">r\nACGT\n")
    base = ["-t", "g.fa", "-p", str(fa), "-o", "out", "-e", "3"]

    def run(args):
        return subprocess.run([SELFTEST, "sam_gapped_options"] + base + args, capture_output=True, text=True)
    full = ["-p2", str(fa), "-sam", "x.sam", "-gapped", "g.tsv"]
    r = run(full + ["-sam_gapped", "1"])
    assert r.returncode == 0 and r.stdout.split() == ["1", "x.sam", "g.tsv"], r.stderr
    assert run(full).stdout.split() == ["0", "x.sam", "g.tsv"]
    assert run(full + ["-sam_gapped", "0"]).stdout.split()[0] == "0"
    assert run(["-p2", str(fa), "-sam_gapped", "0"]).returncode == 0
    for bad, word in ((["-sam", "x.sam", "-gapped", "g.tsv", "-sam_gapped", "1"], "-p2"),
                      (["-p2", str(fa), "-gapped", "g.tsv", "-sam_gapped", "1"], "needs -sam"),
                      (["-p2", str(fa), "-sam", "x.sam", "-sam_gapped", "1"], "needs -gapped"),
                      (full + ["-sam_gapped", "1", "-pairs_all", "1"], "-pairs_all"),
                      (full + ["-sam_gapped"], "missing")):
        r = run(bad)
        assert r.returncode == 1 and word in r.stderr and ("-sam_gapped" in r.stderr or word == "-pairs_all"), (bad, r.stderr)   # (-sam refuses -pairs_all 1 first)
    help_text = subprocess.run([SELFTEST, "options", "-h"], capture_output=True, text=True).stderr
    assert "-sam_gapped" in help_text
    assert "-sam_gapped" in open(os.path.join(ROOT, "README.md")).read()


def _product_records(rlib, pairs, s1, s2):
    out = []
    for src, dt in ((pairs, rlib.PAIR_DTYPE), (s1, rlib.SINGLE_DTYPE), (s2, rlib.SINGLE_DTYPE)):
        t = np.zeros(src.shape[0], dtype=dt)
        for k in dt.names:
            if k in src.dtype.names:
                t[k] = src[k]
        out.append(t)
    return out


def write_selftest_dir(d, genomes, b1, b2, pairs, s1, s2, gaps):
    """what `host_selftest sam_gapped` reads: the records, the ungapped and the gapped lists per genome file, the CIGARs, the mates"""
    import sam_checker as sk
    from real_amd import lib as rlib
    from real_amd import synth
    with open(os.path.join(d, "names.txt"), "w") as f:
        for fi, g in enumerate(genomes):
            for k, name in enumerate(g.frag_names):
                f.write("%d\t%d\t%s\n" % (fi, int(g.frag_start[k]), name))
            f.write("%d\t%d\t\n" % (fi, int(g.frag_start[-1])))
    for arr, name in zip(_product_records(rlib, pairs, s1, s2), ("pairs.bin", "s1.bin", "s2.bin")):
        arr.tofile(os.path.join(d, name))
    fin = sk.final_pairs(pairs, s1, s2)
    for fi, g in enumerate(genomes):
        L, off, _ = sk.mismatch_lists(g.sym, fi, fin, sk.pair_reads(b1, b2))
        L.tofile(os.path.join(d, "mm%d.bin" % fi))
        off.tofile(os.path.join(d, "moff%d.u64" % fi))
        L, off, _ = glc.gapped_lists(g.sym, fi, b1, b2, gaps)
        L.tofile(os.path.join(d, "gmm%d.bin" % fi))
        off.tofile(os.path.join(d, "goff%d.u64" % fi))
    gaps.tofile(os.path.join(d, "gaps.bin"))
    with open(os.path.join(d, "cigars.txt"), "w") as f:
        for i, r in enumerate(gaps):
            b = (b1, b2)[int(gc.target_of(r["tag"]))]
            f.write((gc.cigar_of(r, int(b.offsets[i + 1]) - int(b.offsets[i])) if gc.state_of(r["tag"]) == gc.UNIQUE else "*") + "\n")
    synth.reads_to_fastq(b1, os.path.join(d, "r1"))
    synth.reads_to_fastq(b2, os.path.join(d, "r2"))


def test_host_writer_writes_the_checkers_lines(ora, tmp_path):
    _selftest_built()
    w, pairs, s1, s2, rec = _checked(ora)
    d = str(tmp_path)
    # insert bounds narrower than the run's, so that FLAG 2 is set on some rescued fragments and not on others
    lo, hi = w["min_ins"] + 105, w["max_ins"]
    write_selftest_dir(d, [w["g"]], w["b1"], w["b2"], pairs, s1, s2, rec)
    r = subprocess.run([SELFTEST, "sam_gapped", d, "1", "33", str(lo), str(hi)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-1000:]
    want, ctrs = glc.sam_pairs_gapped([w["g"]], w["b1"], w["b2"], pairs, s1, s2, rec, lo, hi, False)
    got = open(os.path.join(d, "block.sam")).read()
    gl, wl = got.split("\n"), want.split("\n")
    for k, (a, b) in enumerate(zip(gl, wl)):
        assert a == b, (k, a, b)
    assert len(gl) == len(wl)
    rescued = [l.split("\t") for l in wl if "\tZC:i:" in l]
    assert len(rescued) >= 60 and any("D" in f[5] for f in rescued) and any("I" in f[5] for f in rescued)
    assert {int(f[1]) & 2 for f in rescued} == {0, 2}
    assert any(re_follow(f) for f in rescued)


def re_follow(fields):
    import re
    md = [x for x in fields if x.startswith("MD:Z:")][0]
    return re.search(r"\^[A-Z]+0[A-Z]", md) is not None
