"""The indel calls without a GPU: the checker's two formulations of the left shift against each other, the hand cases of the
header and the tie order, the VCF lines by hand, the exports and the mirrors, and the model on the planted workload over the CPU
oracle's records and the checker's rescue."""
import ctypes as C
import os
import subprocess

import numpy as np

import gap_checker as gc
import indel_checker as ic
import indel_workloads as iw
import oracle_lib as ora
import pileup_checker as pk
from abi_header import header_structs
from real_amd import lib as rlib


def _stage(h, min_qual, shift):
    pu = pk.Pileup(h["sym"], 0, min_qual)
    pu.add_pairs(h["pb1"], h["pb2"], h["pairs"])
    ind = ic.Indels(pu, h["frag_start"], shift)
    ind.add(h["b1"], h["b2"], h["gaps"])
    return ind


def test_the_two_formulations_of_the_shift_agree():
    h = iw.hand_cases()
    for min_qual in (0, 20):
        a, b = _stage(h, min_qual, ic.shift_loop), _stage(h, min_qual, ic.shift_run)
        assert a.groups == b.groups and a.stats == b.stats and a.raw == b.raw
        ic.assert_lists_equal(a.events(), b.events())
    # random events over a text of short repeats, both kinds, at every distance from a fragment's start and from an N
    rng = np.random.default_rng(11)
    sym = np.repeat(rng.integers(0, 4, size=400), rng.integers(1, 9, size=400)).astype(np.uint8)
    sym = np.concatenate([sym, np.tile(np.array([0, 1, 2], np.uint8), 200), np.tile(np.array([3], np.uint8), 400)])
    sym[rng.integers(0, sym.shape[0], size=12)] = 4
    n, seen = int(sym.shape[0]), {"shifted": 0, "capped": 0, "n_stop": 0}
    for _ in range(3000):
        g = int(rng.integers(1, 17)) * (1 if rng.random() < 0.5 else -1)
        fs = int(rng.integers(0, n - 40))
        x = int(rng.integers(fs + 1, min(n - 17, fs + 700)))
        if (sym[x - 1:x + max(g, 0)] > 3).any():
            continue
        s = []
        if g < 0:                                                      # half of the insertions copy what stands in front of them
            s = [int(v) & 3 for v in (sym[max(0, x + g):x] if rng.random() < 0.5 and x + g >= 0 else rng.integers(0, 4, size=-g))]
            s = (s + [0] * 16)[:-g]
        one, two = ic.shift_loop(sym, fs, x, g, s), ic.shift_run(sym, fs, x, g, s)
        assert one == two, (fs, x, g, s, one, two)
        seen["shifted"] += one[2] > 0
        seen["capped"] += bool(one[3])
        seen["n_stop"] += one[0] >= 2 and sym[one[0] - 2] > 3
    assert seen["shifted"] > 300 and seen["capped"] > 3 and seen["n_stop"] > 3, seen


def test_what_the_hand_cases_hold():
    h = iw.hand_cases()
    ind = _stage(h, 20, ic.shift_loop)
    st, ev = ind.finish_stats(), ind.events()
    assert h["sym"].shape[0] == iw.HAND_N and len(h["frag_start"]) == 3 and (h["sym"] > 3).sum() >= 40
    got = {}
    for i, note in enumerate(h["what"]):
        got.setdefault(note, []).append(i)
    for note, counter in iw.EMPTY_NOTES.items():
        assert note in got, note
    assert st["invalid"] == sum(v == "invalid" for v in iw.EMPTY_NOTES.values()) and st["on_n"] == 3 and st["other_file"] == 1 and st["ungapped"] == 1
    assert st["low_qual"] == 7 and _stage(h, 0, ic.shift_loop).finish_stats()["low_qual"] == 0
    # splits, gaps, lengths
    rec = h["gaps"]
    lens = np.where(gc.target_of(rec["tag"]) == 0, np.diff(h["b1"].offsets.astype(np.int64)), np.diff(h["b2"].offsets.astype(np.int64)))
    assert {1, 31, 32, 33, 64} <= set(int(j) for j in rec["split"]) and {-16, -15, -1, 1, 16} <= set(int(g) for g in rec["gap"])
    assert {25, 100, 320} <= set(int(l) for l in lens)
    assert any(int(j) == int(l) - 1 - max(-int(g), 0) for j, l, g in zip(rec["split"], lens, rec["gap"]) if g)
    # the shifts: across the word boundaries, to a fragment's first base plus one, to an N, to the cap and exactly to it
    moves = {(x0, x) for _, x0, g, x, _ in ind.raw}
    assert any(x0 > 2048 > x for x0, x in moves) and any(x0 > 3040 > 3008 > x for x0, x in moves)
    assert any(x == iw.HAND_CUT + 1 and x0 > x for x0, x in moves), "a shift that ends at the fragment's first base plus one"
    assert any(x == 5_002 and x0 > x for x0, x in moves), "a shift that ends in front of an N"
    assert any(x0 - x == ic.SHIFT_MAX for x0, x in moves) and st["shift_capped"] >= 8
    assert any(x0 - x == ic.SHIFT_MAX and x0 == 7_256 for x0, x in moves), "256 shifts that the cap does not stop"
    assert any(int(e["pos"]) == iw.HAND_N - 2 for e in ev), "an anchor at n - 2"
    # groups: sizes, one event from both mates and strands with one S, equal position and length but other bases, two kinds at one anchor
    sizes = sorted(int(v) for v in ev["alt_n"])
    assert sizes[-3:] == [64, 65, 300] and 1 in sizes and 2 in sizes
    e7 = [e for e in ev if int(e["gap"]) == -7 and abs(int(e["pos"]) - 999) < 8]
    assert len(e7) == 1 and int(e7[0]["alt_n"]) == 8 and int(e7[0]["alt_fwd"]) == 4
    at = {}
    for e in ev:
        at.setdefault(int(e["pos"]), []).append((int(e["gap"]), int(e["seq"])))
    assert any(len({s for g, s in v if g == -3}) == 2 and any(g == 3 for g, s in v) for v in at.values())


def test_hand_table_and_tie_order():
    assert ic.genotype(10, 10, 300) == (1, 200, 99)
    assert ic.genotype(12, 0, 360) == (2, 317, 33)
    assert ic.genotype(1, 20, 30)[0] == 0
    assert ic.likelihoods(10, 10, 300) == [300, 100, 343] and ic.likelihoods(12, 0, 360) == [360, 76, 43] and ic.likelihoods(1, 20, 30) == [30, 103, 643]
    # ties go to the first of 0/0, 0/1, 1/1
    assert ic.likelihoods(1, 0, 43) == [43, 43, 43] and ic.genotype(1, 0, 43) == (0, 0, 0)        # all three equal: 0/0
    assert ic.genotype(1, 0, 44) == (1, 1, 0)                                                      # [44, 43, 43]: 0/1 before 1/1
    assert ic.likelihoods(2, 0, 43) == [43, 46, 43] and ic.genotype(2, 0, 43) == (0, 0, 0)        # 0/0 before 1/1
    assert ic.genotype(2, 0, 44) == (2, 1, 1)
    assert ic.genotype(9, 1, 1000)[0] == 1 and ic.likelihoods(9, 1, 1000)[1:] == [70, 73]
    # (ref_n 1, alt_n 10: PL(0/1) = 73 = PL(1/1): the heterozygote comes first)
    assert ic.likelihoods(10, 1, 1000)[1:] == [73, 73] and ic.genotype(10, 1, 1000) == (1, 927, 0)
    # the same rows out of the hand-made records
    h = iw.hand_cases()
    ev = _stage(h, 20, ic.shift_loop).events()
    row = {name: [e for e in ev if int(e["pos"]) == x - 1][0] for name, x in h["table"].items()}
    assert [int(row["10/10"][k]) for k in ("ref_n", "alt_n", "qsum", "qual", "gt", "gq")] == [10, 10, 300, 200, 1, 99]
    assert [int(row["12/0"][k]) for k in ("ref_n", "alt_n", "qsum", "qual", "gt", "gq")] == [0, 12, 360, 317, 2, 33]
    assert [int(row["1/20"][k]) for k in ("ref_n", "alt_n", "qsum", "gt")] == [20, 1, 30, 0]


def test_vcf_lines_by_hand():
    sym = np.array([0, 1, 2, 3, 3, 0, 1, 1, 2, 0, 3, 2], dtype=np.uint8)             # ACGTTACCGATG
    frag_start, names = [0, 5, 12], ["chrA", "chrB"]
    dele = np.zeros(1, dtype=ic.INDEL_DTYPE)[0]
    dele["pos"], dele["ref_n"], dele["alt_n"], dele["alt_fwd"], dele["qual"], dele["gap"], dele["gt"], dele["gq"], dele["ref"] = 6, 10, 10, 6, 200, 2, 1, 99, 1
    assert ic.vcf_line(dele, sym, frag_start, names) == "chrB\t2\t.\tCCG\tC\t200\t.\tDP=20;INDEL;SF=6;SR=4\tGT:GQ:DP:AD\t0/1:99:20:10,10\n"
    ins = np.zeros(1, dtype=ic.INDEL_DTYPE)[0]
    ins["pos"], ins["alt_n"], ins["alt_fwd"], ins["qual"], ins["gap"], ins["gt"], ins["gq"], ins["ref"] = 1, 12, 5, 317, -3, 2, 33, 1
    ins["seq"] = ic.pack_seq([3, 0, 2])
    assert ic.vcf_line(ins, sym, frag_start, names) == "chrA\t2\t.\tC\tCTAG\t317\t.\tDP=12;INDEL;SF=5;SR=7\tGT:GQ:DP:AD\t1/1:33:12:0,12\n"
    assert ic.unpack_seq(ic.pack_seq([3, 0, 2, 1] * 4), 16) == [3, 0, 2, 1] * 4 and ic.pack_seq([3] * 16) == 0xffffffff
    head = ic.vcf_header([("chrA", 5), ("chrB", 7)])
    assert head.count("##INFO") == 4 and "ID=INDEL,Number=0,Type=Flag" in head and head.index("ID=DP,") < head.index("ID=INDEL") < head.index("ID=SF") < \
        head.index("ID=SR") < head.index("##FORMAT")
    # merged by position, the SNP first at an equal one
    import call_checker as ck
    snp = np.zeros(2, dtype=ck.CALL_DTYPE)
    snp["pos"], snp["ref"], snp["a1"], snp["a2"] = [1, 8], [1, 2], [1, 0], [3, 0]
    indels = np.array([ins, dele], dtype=ic.INDEL_DTYPE)
    pos = [l.split("\t")[:2] + [l.split("\t")[7].count("INDEL")] for l in ic.vcf_lines_merged(snp, indels, sym, frag_start, names).splitlines()]
    assert pos == [["chrA", "2", 0], ["chrA", "2", 1], ["chrB", "2", 1], ["chrB", "4", 0]]


def test_exports_record_and_mirrors():
    L = rlib.load()
    for name in ("real_hip_indel_begin", "real_hip_indel_add", "real_hip_indel_finish", "real_hip_indel_events", "real_hip_indel_calls",
                 "real_hip_indel_end", "real_hip_indel_stats_get"):
        assert name in rlib.ABI_SYMBOLS and hasattr(L, name), name
    hs = header_structs()
    assert hs["real_hip_indel"] == list(ic.INDEL_DTYPE.names) == [f for f, _ in rlib.RealHipIndel._fields_]
    assert C.sizeof(rlib.RealHipIndel) == 32 and rlib.INDEL_DTYPE == ic.INDEL_DTYPE
    assert [rlib.INDEL_DTYPE.fields[f][1] for f in rlib.INDEL_DTYPE.names] == [ic.INDEL_DTYPE.fields[f][1] for f in ic.INDEL_DTYPE.names]
    assert hs["real_hip_indel_params"] == [f for f, _ in rlib.RealHipIndelParams._fields_] == ["struct_size", "min_call_qual", "min_alt", "min_depth"]
    assert hs["real_hip_indel_stats"][2:] == list(rlib.INDEL_STATS_FIELDS) == list(ic.COUNTERS) + ["distinct", "calls", "het", "hom", "deletions", "insertions",
                                                                                                   "launches", "kernel_ms"]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(rlib.__file__))), "include", "real_hip.h")).read()
    for name, value in (("REAL_HIP_INDEL_SHIFT_MAX", ic.SHIFT_MAX), ("REAL_HIP_INDEL_REF_Q", ic.REF_Q), ("REAL_HIP_INDEL_PRIOR_HET", ic.PRIOR_HET),
                        ("REAL_HIP_INDEL_PRIOR_HOM", ic.PRIOR_HOM), ("REAL_HIP_ABI_VERSION", 2)):
        assert "#define %s %du" % (name, value) in " ".join(hdr.split()) or "#define %s %d" % (name, value) in " ".join(hdr.split()), name
    assert (rlib.INDEL_SHIFT_MAX, rlib.INDEL_REF_Q, rlib.INDEL_PRIOR_HET, rlib.INDEL_PRIOR_HOM) == (ic.SHIFT_MAX, ic.REF_Q, ic.PRIOR_HET, ic.PRIOR_HOM)
    assert ic.PRIOR_HET == rlib.CALL_PRIOR_HET + 10 and ic.PRIOR_HOM == rlib.CALL_PRIOR_HOM + 10 and ic.HET == rlib.CALL_HET


def test_the_model_on_the_planted_workload():
    """At least 90 % of the planted indels that at least 8 rescued mates show are called with the planted genotype (DESIGN.md 7e's
    condition); measured: 21 of 23 (91.3 %), 3 unplanted calls."""
    w = iw.planted()
    assert int(w.g.frag_start.shape[0]) == 3 and abs(w.b1.n_reads * 200 / w.g.n - iw.P_DEPTH) < 2
    assert {abs(p["g"]) for p in w.plants} == set(range(1, 9)) and {p["cls"] for p in w.plants} == set(iw.P_CLASSES)
    pairs, s1, s2, _ = iw.oracle_records(ora, w)
    gaps, ctr = gc.check_gap(gc.Text(w.g.sym, w.g.frag_start, 0), w.b1, w.b2, pairs, s1, s2, w.min_ins, w.max_ins, w.prm)
    pu = pk.Pileup(w.g.sym, 0, 20)
    pu.add_pairs(w.b1, w.b2, pairs)
    ind = ic.Indels(pu, w.g.frag_start)
    ind.add(w.b1, w.b2, gaps)
    ev = {(int(e["pos"]), int(e["gap"]), int(e["seq"])): e for e in ind.events()}
    # the coverage floors: events per class, per target mate and per strand
    by_class, by_mate, by_strand = dict.fromkeys(iw.P_CLASSES, 0), [0, 0], [0, 0]
    keys = {iw.planted_key(w, p): p for p in w.plants}
    for i, x0, g, x, seq in ind.raw:
        p = keys.get((x - 1, g, seq))
        if p is not None:
            by_class[p["cls"]] += 1
            by_mate[int(gc.target_of(gaps["tag"][i]))] += 1
            by_strand[int(gc.inverted_of(gaps["tag"][i]))] += 1
    assert min(by_class.values()) >= 5 and min(by_mate) >= 5 and min(by_strand) >= 5, (by_class, by_mate, by_strand)
    shown = [p for p in w.plants if iw.planted_key(w, p) in ev and int(ev[iw.planted_key(w, p)]["alt_n"]) >= 8]
    right = [p for p in shown if int(ev[iw.planted_key(w, p)]["gt"]) == (2 if p["hom"] else 1)]
    unplanted = sum(1 for k, e in ev.items() if int(e["gt"]) and k not in keys)
    print("planted indels shown by >= 8 mates: %d, called with the planted genotype: %d, unplanted calls: %d" % (len(shown), len(right), unplanted))
    assert len(shown) >= 20 and len(right) >= 0.9 * len(shown), (len(right), len(shown))


# ---- the command line's side, without a GPU: the parser and the VCF writer -------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "real_amd", "host", "host_selftest")


def _selftest_built():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "real_amd", "host"), "host_selftest"], stdout=subprocess.DEVNULL)


def test_realoptions_vcf_indels_flags_and_loud_refusals(tmp_path):
    """-vcf_indels / -vcf_minalt through the C++ parser (host_selftest vcf_indel_options): what they need, loudly, before any file is read"""
    _selftest_built()
    fa = tmp_path / "m2.fa"
    fa.write_text(">r\nACGT\n")
    base = ["-t", "no_such_genome.fa", "-p", str(fa), "-o", "out", "-e", "3"]

    def run(args):
        return subprocess.run([SELFTEST, "vcf_indel_options"] + base + args, capture_output=True, text=True)
    full = ["-p2", str(fa), "-vcf", "x.vcf"]
    assert run(full + ["-vcf_indels", "1"]).stdout.split() == ["1", "2", "20", "4"]
    assert run(full + ["-vcf_indels", "1", "-vcf_minalt", "5", "-vcf_minqual", "30", "-vcf_mindepth", "9"]).stdout.split() == ["1", "5", "30", "9"]
    assert run(full).stdout.split() == ["0", "2", "20", "4"] and run(full + ["-vcf_indels", "0"]).stdout.split()[0] == "0"
    for bad, word in ((["-p2", str(fa), "-vcf_indels", "1"], "needs -vcf"), (["-vcf", "x.vcf", "-vcf_indels", "1"], "-p2"),
                      (full + ["-vcf_minalt", "3"], "only meaningful with -vcf_indels 1"), (full + ["-vcf_indels", "0", "-vcf_minalt", "3"], "-vcf_indels 1"),
                      (full + ["-vcf_indels", "1", "-vcf_minalt", str(1 << 32)], "2^32"), (full + ["-vcf_indels"], "missing")):
        r = run(bad)
        assert r.returncode == 1 and word in r.stderr and ("-vcf_indels" in r.stderr or "-vcf_minalt" in r.stderr), (bad, r.stderr)
    help_text = subprocess.run([SELFTEST, "options", "-h"], capture_output=True, text=True).stderr
    assert "-vcf_indels" in help_text and "-vcf_minalt" in help_text and "do NOT reach the rescued mates" in help_text
    assert "-vcf_indels" in open(os.path.join(ROOT, "README.md")).read()


def test_the_vcf_writer_against_the_checkers_lines(tmp_path):
    """host_selftest vcf_indels: Vcf.hpp's header and merged lines from records on disk are the checker's, byte for byte"""
    import call_checker as ck
    _selftest_built()
    h = iw.hand_cases()
    pu = pk.Pileup(h["sym"], 0, 20)
    pu.add_pairs(h["pb1"], h["pb2"], h["pairs"])
    ind = ic.Indels(pu, h["frag_start"])
    ind.add(h["b1"], h["b2"], h["gaps"])
    indels = ind.calls(20, 2, 0)
    wide = np.zeros(2, dtype=ic.INDEL_DTYPE)                          # the widest gaps, by hand: 16 deleted bases, 16 inserted ones
    wide["pos"], wide["gap"], wide["seq"], wide["gt"], wide["alt_n"], wide["alt_fwd"], wide["ref_n"] = [30_000, 30_500], [16, -16], [0, 0xDEADBEEF], [2, 1], 9, 4, [0, 7]
    wide["ref"] = [int(pu.ref[30_000]), int(pu.ref[30_500])]
    indels = np.concatenate([indels, wide])
    indels = indels[np.argsort(indels["pos"], kind="stable")]
    # SNP records by hand: in front of, at and behind indel anchors, in both fragments
    at = sorted({int(indels["pos"][0]), int(indels["pos"][3]) - 1, int(indels["pos"][5]) + 1, int(indels["pos"][-1]), 5, iw.HAND_CUT, iw.HAND_N - 1})
    snp = np.zeros(len(at), dtype=ck.CALL_DTYPE)
    for k, x in enumerate(at):
        ref = int(pu.ref[x])
        snp[k] = (x, 9 + k, [1 + k, 2, 3, 4], 50 + k, ref, 0, 0, 40)
        snp["a1"][k], snp["a2"][k] = sorted((ref if k & 1 else (ref + 1) & 3, (ref + 1) & 3))
    names = ["first", "second"]
    d = str(tmp_path)
    h["sym"].tofile(os.path.join(d, "sym.u8"))
    np.asarray(h["frag_start"], dtype=np.uint64).tofile(os.path.join(d, "frag.u64"))
    snp.tofile(os.path.join(d, "calls.bin"))
    indels.tofile(os.path.join(d, "indels.bin"))
    open(os.path.join(d, "names.txt"), "w").write("".join(n + "\n" for n in names))
    r = subprocess.run([SELFTEST, "vcf_indels", d], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    contigs = [(names[k], int(h["frag_start"][k + 1] - h["frag_start"][k])) for k in range(2)]
    want = ic.vcf_header(contigs) + ic.vcf_lines_merged(snp, indels, h["sym"], h["frag_start"], names)
    got = open(os.path.join(d, "out.vcf")).read()
    assert got == want
    lines = [l.split("\t") for l in got.splitlines() if not l.startswith("#")]
    assert len(lines) == len(at) + indels.shape[0] and sum("INDEL" in l[7] for l in lines) == indels.shape[0] > 20
    assert any(len(l[3]) == 17 for l in lines) and any(len(l[4]) == 17 for l in lines), "a deletion and an insertion of 16 bases"
    same = [k for k in range(len(lines) - 1) if lines[k][:2] == lines[k + 1][:2]]
    assert same and all("INDEL" not in lines[k][7] or "INDEL" in lines[k + 1][7] for k in same), "the SNP line first at an equal POS"
    assert {l[0] for l in lines} == set(names)
