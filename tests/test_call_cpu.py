"""The variant calls without a GPU: the checker (call_checker.py) on the hand values of include/real_hip.h and DESIGN.md 7e, the
tie order, what the shared workload (call_workloads.py) must contain and the model's sanity on it -- judged on the checker
and the oracle's records alone -- and the parts of the library and of the command line that need no device: the exported
symbols, the records' sizes, and the loud errors of `real`."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np

import call_checker as ck
import call_workloads as cw
import pileup_checker as pk
import pileup_workloads as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "real_amd", "host", "real")
A, Cb, G, T = 0, 1, 2, 3


def _site(counts, q=30):
    """cnt / qsum of a site where base b was seen counts[b] times, every time with quality q"""
    cnt = [counts.get(b, 0) for b in range(4)]
    return cnt, [q * c for c in cnt]


# ---- the hand table (ref = A, all qualities 30) ---------------------------------------------------------------------
def test_hand_values():
    cnt, qs = _site({A: 10, Cb: 10})
    pl = dict(zip(ck.genotype_order(A), ck.likelihoods(A, cnt, qs)))
    assert pl[(A, Cb)] == 90 and pl[(A, A)] == 350
    assert ck.genotype(A, cnt, qs) == (A, Cb, 260, 99)
    cnt, qs = _site({Cb: 20})
    pl = dict(zip(ck.genotype_order(A), ck.likelihoods(A, cnt, qs)))
    assert pl[(Cb, Cb)] == 33 and pl[(A, Cb)] == 90 and pl[(A, A)] == 700
    assert ck.genotype(A, cnt, qs) == (Cb, Cb, 667, 57)
    cnt, qs = _site({A: 17, Cb: 3})
    pl = dict(zip(ck.genotype_order(A), ck.likelihoods(A, cnt, qs)))
    assert pl[(A, A)] == 105 and pl[(A, Cb)] == 90
    assert ck.genotype(A, cnt, qs)[:3] == (A, Cb, 15)                  # no call at the default min_call_qual 20
    assert ck.genotype(A, *_site({A: 16, Cb: 4}))[:3] == (A, Cb, 50)
    assert ck.genotype(A, *_site({A: 19, Cb: 1}))[:2] == (A, A)         # hom-ref best: no call
    # two other bases: C10 G10 over A -- C/G costs 60 + 60, hom-C 350 + 33, a heterozygote with A 30 + 30 + 350
    assert ck.genotype(A, *_site({Cb: 10, G: 10})) == (Cb, G, 700 - 120, 99)
    assert ck.genotype(A, [0, 0, 0, 0], [0, 0, 0, 0]) == (A, A, 0, 30)  # nothing seen: the prior alone


def test_tie_order():
    """(ref, ref) first, then the other nine by ascending (a, b); the best is the first of minimal PL"""
    assert ck.genotype_order(G) == [(G, G), (A, A), (A, Cb), (A, G), (A, T), (Cb, Cb), (Cb, G), (Cb, T), (G, T), (T, T)]
    # (ref, ref) against a heterozygote: PL(G,G) = E[A] = 33 + 15, PL(A,G) = 3 * 6 + 30
    cnt, qs = [3, 0, 3, 0], [33, 0, 90, 0]
    pl = dict(zip(ck.genotype_order(G), ck.likelihoods(G, cnt, qs)))
    assert pl[(G, G)] == pl[(A, G)] == 48
    assert ck.genotype(G, cnt, qs) == (G, G, 0, 0)                      # the tie goes to (ref, ref), which stands first; GQ 0
    # a tie between two heterozygotes that hold ref: A and T seen alike over G -- (A, G) stands before (G, T)
    cnt, qs = [5, 0, 5, 5], [150, 0, 150, 150]
    pl = dict(zip(ck.genotype_order(G), ck.likelihoods(G, cnt, qs)))
    assert pl[(A, G)] == pl[(G, T)] and pl[(A, T)] == pl[(A, G)] + 30
    assert ck.genotype(G, cnt, qs)[:2] == (A, G) and ck.genotype(G, cnt, qs)[3] == 0
    # and between (A, A) and (A, C) over ref G, the homozygote stands first: PL(A,A) = E[C] + 33, PL(A,C) = 3 (cA + cC) + 60
    cnt, qs = [10, 11, 0, 0], [300, 5, 0, 0]                            # E[C] = 60, hom-A 93; A/C 63 + 60
    assert ck.likelihoods(G, cnt, qs)[1] == 93 and ck.likelihoods(G, cnt, qs)[2] == 123
    cnt, qs = [3, 4, 0, 0], [90, 28, 0, 0]                              # E[C] = 48: hom-A 81; A/C 21 + 60 = 81
    pl = ck.likelihoods(G, cnt, qs)
    assert pl[1] == pl[2] == 81 and ck.genotype(G, cnt, qs)[:2] == (A, A)


def test_checker_evidence_by_hand():
    """ACGTNNTGCA: evidence is taken at the pileup's sites only, the reference base included, quality-filtered by the strand"""
    genome = np.array([0, 1, 2, 3, 4, 4, 3, 2, 1, 0], dtype=np.uint8)
    reads = [[0, 1, 1, 3], [0, 1, 2, 3], [0, 1, 1, 3], [2, 1, 0, 3]]   # ACCT, ACGT, ACCT forward at 0; GCAT reverse at 6 = ATGC over TGCA
    quals = [[40, 40, 30, 40], [40, 40, 25, 40], [40, 40, 10, 40], [5, 40, 40, 40]]
    info = np.array([(1 << 61) | 0, (1 << 61) | 0, (1 << 61) | 0, (2 << 61) | 6], dtype=np.uint64)
    off = np.arange(0, 17, 4).astype(np.uint64)
    b = types.SimpleNamespace(bases=np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]), qual=np.concatenate([np.asarray(q, dtype=np.uint8) for q in quals]), offsets=off)
    pu = pk.Pileup(genome, 0, 20)
    pu.add(b, info)
    assert pu.sites()["pos"].tolist() == [2, 6, 7, 8]                  # (9: the reverse read's base 0 has quality 5)
    cl = ck.Calls(pu)
    cl.add(b, info)
    e = cl.evidence()
    assert e["cnt"][0].tolist() == [0, 1, 1, 0] and e["qsum"][0].tolist() == [0, 30, 25, 0]     # the third C has quality 10
    assert e["cnt"][1].tolist() == [1, 0, 0, 0] and e["qsum"][1].tolist() == [40, 0, 0, 0]
    assert cl.stats == dict(reads=4, placed=4, other_file=0, invalid=0, site_bases=5, low_qual=1)
    for s, site in enumerate(pu.sites()):                               # the cross-check between the two passes
        for base in range(4):
            assert base == site["ref"] or e["cnt"][s][base] == site["alt"][base]
    c = cl.calls(min_call_qual=0, min_depth=1)
    # one base each: the homozygote of it (33) ties with the heterozygote that holds ref (3 + 30), and the one that stands first wins:
    # over T, (A, A) before (A, T); over G, (G, T) before (T, T); over C, (C, G) before (G, G)
    assert c["pos"].tolist() == [6, 7, 8] and c["a1"].tolist() == [0, 2, 1] and c["a2"].tolist() == [0, 3, 2] and c["gq"].tolist() == [0, 0, 0]
    assert ck.vcf_lines(c[:1], [0, 10], ["g"]) == "g\t7\t.\tT\tA\t12\t.\tDP=1\tGT:GQ:DP:AD\t1/1:0:1:0,1\n"
    assert cl.finish_stats(0, 1)["hom"] == 1 and cl.finish_stats(0, 1)["het"] == 2 and cl.finish_stats(0, 2)["calls"] == 0 and cl.finish_stats(13, 1)["calls"] == 0


def test_vcf_lines_by_hand():
    calls = np.zeros(3, dtype=ck.CALL_DTYPE)
    calls["pos"], calls["depth"], calls["qual"], calls["gq"] = [4, 12, 13], [40, 41, 42], [260, 667, 50], [99, 57, 7]
    calls["cnt"] = [[10, 10, 0, 1], [0, 20, 0, 0], [1, 9, 2, 9]]
    calls["ref"], calls["a1"], calls["a2"] = [0, 0, 2], [0, 1, 1], [1, 1, 3]
    assert ck.vcf_lines(calls, [0, 10, 20], ["x", "y"]) == (
        "x\t5\t.\tA\tC\t260\t.\tDP=40\tGT:GQ:DP:AD\t0/1:99:21:10,10\n"
        "y\t3\t.\tA\tC\t667\t.\tDP=41\tGT:GQ:DP:AD\t1/1:57:20:0,20\n"
        "y\t4\t.\tG\tC,T\t50\t.\tDP=42\tGT:GQ:DP:AD\t1/2:7:21:2,9,9\n")
    calls["ref"][0], calls["a1"][0], calls["a2"][0] = 1, 0, 1          # ref C, genotype A/C: the reference allele is index 0
    assert ck.vcf_lines(calls[:1], [0, 10], ["x"]).split("\t")[3:5] == ["C", "A"] and "\t0/1:99:21:10,10\n" in ck.vcf_lines(calls[:1], [0, 10], ["x"])
    head = ck.vcf_header([("x", 10), ("y", 10)])
    assert head.startswith("##fileformat=VCFv4.2\n##contig=<ID=x,length=10>\n##contig=<ID=y,length=10>\n##INFO=<ID=DP,")
    assert head.endswith("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tsample\n") and head.count("##FORMAT=<ID=") == 4


# ---- what the workload must contain, and the model's sanity on it ---------------------------------------------------
def test_workload_and_model_sanity(ora):
    w = cw.workload()
    n, (lo, hi) = w.g.n, pw.N_RUN
    assert sum(1 for a, b in w.planted.values() if a == b) == cw.N_HOM and len(w.planted) == cw.N_HOM + cw.N_HET
    at = set(w.planted)
    assert {0, n - 1, lo - 1, hi} <= at and {x % 64 for x in at} >= {0, 63, 31, 32} and {x % 32 for x in at} >= {0, 31}
    lens = {k: (getattr(w, k).offsets[1:] - getattr(w, k).offsets[:-1]).astype(np.int64) for k in cw.BATCHES}
    assert lens["ragged"].min() == 33 and lens["ragged"].max() == 320 and lens["long"].min() == 321 and lens["long"].max() == 700
    ends_at_n = False
    for k in cw.BATCHES:
        st, _, _, _, pos = ora.unpack_record(cw.oracle_records(ora, k))
        placed = (st == 1) | (st == 2)
        print("%s: %d reads, %d placed (%d forward, %d reverse)" % (k, len(st), placed.sum(), (st == 1).sum(), (st == 2).sum()))
        assert placed.sum() >= 0.9 * len(st) and (st == 1).sum() >= placed.sum() / 4 and (st == 2).sum() >= placed.sum() / 4
        ends_at_n = ends_at_n or bool((pos[placed] + lens[k][placed] == n).any())
    assert ends_at_n
    pu, cl = cw.expected(ora, cw.BATCHES, 20)
    assert pu.stats["n_dropped"] == 0 and pu.stats["invalid"] == 0 and pu.finish_stats()["max_depth"] >= 300
    assert cl.stats["placed"] == pu.stats["placed"] > 20_000 and cl.stats["low_qual"] > 10_000
    print("mean depth %.1f, %d sites, %d site bases" % (pu.stats["bases"] / n, cl.site_list.shape[0], cl.stats["site_bases"]))
    # the cross-check between the two passes, on the checker itself
    other = np.arange(4)[None, :] != cl.site_list["ref"][:, None].astype(np.int64)
    assert (cl.cnt[other] == cl.site_list["alt"].astype(np.int64)[other]).all()
    # of the planted substitutions with unfiltered depth >= 25, at least 90 % are called with the planted genotype
    calls = cl.calls()                                                  # the defaults of `real -vcf`: QUAL >= 20, DP >= 4
    by_pos = {int(c["pos"]): (int(c["a1"]), int(c["a2"])) for c in calls}
    deep = [x for x in w.planted if pu.depth[x] >= 25]
    right = [x for x in deep if by_pos.get(x) == w.planted[x]]
    het = [x for x in deep if w.planted[x][0] != w.planted[x][1]]
    print("planted: %d, of depth >= 25: %d (%d het, %d hom); called with the planted genotype: %d (%d het, %d hom)" % (
        len(w.planted), len(deep), len(het), len(deep) - len(het), len(right), len(set(right) & set(het)), len(set(right) - set(het))))
    assert len(deep) >= 150 and {0, n - 1, lo - 1, hi, pw.HOT_AT + 40} <= set(deep)
    assert len(right) >= 0.9 * len(deep)
    unplanted = [x for x in by_pos if x not in w.planted]
    print("calls at unplanted positions: %d of %d calls (%d sites)" % (len(unplanted), calls.shape[0], cl.site_list.shape[0]))


# ---- the library and the command line, without a device -------------------------------------------------------------
SYMBOLS = ["real_hip_call_begin", "real_hip_call_add", "real_hip_call_add_pairs", "real_hip_call_finish", "real_hip_call_evidence",
           "real_hip_call_variants", "real_hip_call_end", "real_hip_call_stats_get"]


def test_library_exports_the_calls():
    """the symbols are looked up in a child process: this file runs before every GPU test of the suite, and a process that has
    loaded the library before PyTorch brought its HIP runtime up is not one to run them in (conftest.py)"""
    from real_amd import lib as rlib
    code = ("import sys; sys.path.insert(0, %r); from real_amd import lib; L = lib.load(); "
            "print([n for n in %r if not hasattr(L, n)], L.real_hip_abi_version())" % (ROOT, SYMBOLS))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0 and r.stdout.decode().strip() == "[] 2", (r.stdout.decode(), r.stderr.decode()[-1000:])
    for name in SYMBOLS:
        assert name in rlib.ABI_SYMBOLS, name
    assert rlib.CALL_EVIDENCE_DTYPE.itemsize == 32 and rlib.CALL_DTYPE.itemsize == 32
    assert rlib.CALL_EVIDENCE_DTYPE == ck.EVIDENCE_DTYPE and rlib.CALL_DTYPE == ck.CALL_DTYPE
    assert C.sizeof(rlib.RealHipCallParams) == 12 and C.sizeof(rlib.RealHipCallStats) == 8 + 11 * 8
    assert (rlib.CALL_HET, rlib.CALL_ERR, rlib.CALL_PRIOR_HET, rlib.CALL_PRIOR_HOM, rlib.CALL_PRIOR_HET2) == (ck.HET, ck.ERR, ck.PRIOR_HET, ck.PRIOR_HOM, ck.PRIOR_HET2)
    header = open(os.path.join(ROOT, "include", "real_hip.h")).read()
    for name, value in (("HET", 3), ("ERR", 5), ("PRIOR_HET", 30), ("PRIOR_HOM", 33), ("PRIOR_HET2", 60)):      # named once
        assert re.findall(r"#define\s+REAL_HIP_CALL_%s\s+(\d+)u\b" % name, header) == [str(value)], name


def test_real_refuses_vcf_flags_that_cannot_work(tmp_path):
    """each before anything runs (no device is needed), non-zero, with a message of its own that names the flag"""
    fa, fq, fq2 = str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), str(tmp_path / "r2.fq")
    open(fa, "w").write(">g\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    for f in (fq, fq2):
        open(f, "w").write("@r\nACGTACGTACGTACGTACGTACGTACGTACGTAC\n+\n" + "I" * 34 + "\n")
    out, vf, pf, sf = str(tmp_path / "o.tsv"), str(tmp_path / "v.vcf"), str(tmp_path / "p.tsv"), str(tmp_path / "s.sam")
    base = [REAL, "-t", fa, "-p", fq, "-o", out]
    cases = [(base + ["-vcf", vf, "-u", "0"], b"-vcf calls variants from the unique placements: it cannot be combined with -u 0"),
             (base + ["-p2", fq2, "-vcf", vf, "-pairs_all", "1"], b"-vcf calls variants from the unique placement of a fragment: it cannot be combined with -pairs_all 1"),
             (base + ["-vcf_minqual", "30"], b"-vcf_minqual is only meaningful with -vcf"),
             (base + ["-pileup", pf, "-vcf_mindepth", "8"], b"-vcf_mindepth is only meaningful with -vcf"),
             (base + ["-vcf", out], b"same file as -o"), (base + ["-vcf", "-"], b"standard output (-) cannot be it"), (base + ["-vcf", ""], b"needs a file name"),
             (base + ["-vcf", pf, "-pileup", pf], b"same file as -pileup"), (base + ["-vcf", pf, "-pileup_depth", pf], b"same file as -pileup"),
             (base + ["-vcf", sf, "-sam", sf], b"same file as -sam"),
             (base + ["-pileup_minq", "20"], b"-pileup_minq is only meaningful with -pileup"),
             (base + ["-vcf", vf, "-pileup_minq", "64"], b"-pileup_minq takes a quality of at most 63")]
    for args, word in cases:
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode != 0 and word in r.stderr and b"unknown argument" not in r.stderr, (args, r.stderr.decode()[-600:])
        assert not any(os.path.exists(f) for f in (vf, pf, sf, out))
    r = subprocess.run([REAL, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    for word in (b"-vcf <file", b"-vcf_minqual <Q", b"-vcf_mindepth <D"):
        assert word in r.stderr, word
