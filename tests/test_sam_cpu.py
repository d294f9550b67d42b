"""The mismatch lists and the SAM lines without a GPU: the checker (sam_checker.py) on hand-made cases, every placed line of
the shared workload rebuilt into the genome from SEQ + MD alone, and the parts of the library and of the command line that
need no device: the exported symbols, the 4-byte record, the statistics struct, and the loud errors of `real`."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

import pileup_workloads as pw
import sam_checker as sk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "real_amd", "host", "real")


def _info(state, pos, fileid=0, frag=0, errors=0):
    return (state << 61) | (frag << 45) | (errors << 41) | (fileid << 35) | pos


def _batch(reads):
    off = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    return types.SimpleNamespace(bases=np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]), offsets=off, n_reads=len(reads),
                                 qual=np.concatenate([np.arange(len(r), dtype=np.uint8) for r in reads]), ids=["r%d extra" % i for i in range(len(reads))])


#                 0  1  2  3  4  5  6  7  8  9
GENOME = np.array([0, 1, 2, 3, 4, 4, 3, 2, 1, 0], dtype=np.uint8)      # ACGTNNTGCA


def _lists(reads, info, fileid=0):
    b = _batch(reads)
    return sk.mismatch_lists(GENOME, fileid, sk.final_single(np.array(info, dtype=np.uint64)), sk.single_reads(b))


def _rows(L):
    return [(int(e["off"]), int(e["ref"]), int(e["base"])) for e in L]


# ---- the checker, by hand -------------------------------------------------------------------------------------------
def test_checker_forward_and_reverse_read():
    # ACGT at 0 with its third base wrong: offset 2, the text's G, the read's A
    L, off, st = _lists([[0, 1, 0, 3]], [_info(1, 0, errors=1)])
    assert _rows(L) == [(2, 2, 0)] and off.tolist() == [0, 1]
    assert st == dict(reads=1, placed=1, other_file=0, invalid=0, bases=4, mismatches=1, on_n=0, disagree=0)
    # the reverse strand at 6 (text TGCA): the read TGCC oriented is GGCA -> offset 0, the text's T, the oriented read's G
    L, off, st = _lists([[3, 2, 1, 1]], [_info(2, 6, errors=1)])
    assert _rows(L) == [(0, 3, 2)] and st["disagree"] == 0
    # a perfect read on either strand: an empty list
    L, off, st = _lists([[0, 1, 2, 3], [3, 2, 1, 0]], [_info(1, 0), _info(2, 6)])
    assert L.shape[0] == 0 and off.tolist() == [0, 0, 0] and st["placed"] == 2 and st["bases"] == 8


def test_md_at_the_first_base_the_last_base_and_two_adjacent_ones():
    L, _, _ = _lists([[1, 1, 2, 3]], [_info(1, 0, errors=1)])          # offset 0
    assert sk.md_of(L, 4) == "0A3"
    L, _, _ = _lists([[0, 1, 2, 0]], [_info(1, 0, errors=1)])          # offset L - 1
    assert sk.md_of(L, 4) == "3T0"
    L, _, _ = _lists([[1, 0, 2, 3]], [_info(1, 0, errors=2)])          # offsets 0 and 1
    assert sk.md_of(L, 4) == "0A0C2" and _rows(L) == [(0, 0, 1), (1, 1, 0)]
    L, _, _ = _lists([[0, 1, 2, 3]], [_info(1, 0)])
    assert sk.md_of(L, 4) == "4"
    for seq, md, ref in (("CCGT", "0A3", "ACGT"), ("ACGA", "3T0", "ACGT"), ("CAGT", "0A0C2", "ACGT"), ("ACGT", "4", "ACGT")):
        assert sk.reference_from_md(seq, md) == ref


def test_checker_placement_over_an_n():
    # positions 2..7 = G T N N T G; the read shows G T A C T G: both N are listed with ref 4, whatever the read shows
    L, off, st = _lists([[2, 3, 0, 1, 3, 2]], [_info(1, 2, errors=0)])
    assert _rows(L) == [(2, 4, 0), (3, 4, 1)] and st["on_n"] == 2 and st["mismatches"] == 2 and st["disagree"] == 1
    assert sk.md_of(L, 6) == "2N0N2"


def test_checker_other_file_invalid_and_other_states():
    reads = [[0, 1, 2, 3], [0, 1, 2, 3], [2, 1, 0], [0, 1, 2, 3], [0, 1, 2, 3]]
    info = [_info(1, 0, fileid=1), _info(1, 0), _info(1, 8), _info(4, 0), _info(0, 0)]      # another file; placed; behind the text; NonUnique; NoMatch
    L, off, st = _lists(reads, info)
    assert st == dict(reads=5, placed=1, other_file=1, invalid=1, bases=4, mismatches=0, on_n=0, disagree=0) and off.tolist() == [0] * 6
    # a placement that ends exactly at n is valid
    L, off, st = _lists([[1, 0]], [_info(1, 8)])
    assert st["placed"] == 1 and st["invalid"] == 0


def _pair(state, pos1, pos2, inv1, k1=0, k2=0):
    p = np.zeros(1, dtype=np.dtype([("best", "<f8"), ("second", "<f8"), ("pos1", "<u4"), ("pos2", "<u4"), ("score1", "<f4"), ("score2", "<f4"),
                                    ("frag", "<u2"), ("fileid", "u1"), ("k1", "u1"), ("k2", "u1"), ("inverted1", "u1"), ("state", "u1"), ("reserved", "u1")]))
    p["state"], p["pos1"], p["pos2"], p["inverted1"], p["k1"], p["k2"] = state, pos1, pos2, inv1, k1, k2
    return p


def _single(state, pos, inv, k=0):
    s = np.zeros(1, dtype=np.dtype([("score", "<f4"), ("second", "<f4"), ("pos", "<u4"), ("frag", "<u2"), ("fileid", "u1"), ("tag", "u1")]))
    s["pos"], s["tag"] = pos, k | (inv << 4) | (state << 5)
    return s


def test_checker_pairs_with_and_without_singles():
    b1, b2 = _batch([[0, 1, 2, 0]]), _batch([[3, 2, 1, 0]])             # mate 1 ACGA forward at 0, mate 2 TGCA forward at 6
    s1, s2 = _single(1, 0, 0, 1), _single(1, 6, 0)
    reads = sk.pair_reads(b1, b2)
    # a Unique pair: mate 1 at pos1 on inverted1, mate 2 at pos2 on the other strand (TGCA turned round is TGCA)
    fin = sk.final_pairs(_pair(1, 0, 6, 0, k1=1), s1, s2)
    assert fin.placed.tolist() == [True, True] and fin.inv.tolist() == [False, True] and fin.paired.all()
    L, off, st = sk.mismatch_lists(GENOME, 0, fin, reads)
    assert _rows(L) == [(3, 3, 0)] and off.tolist() == [0, 1, 1] and st["reads"] == 2 and st["placed"] == 2 and st["disagree"] == 0
    # NoMatch with singles: each mate's own Unique record; without singles: nothing
    fin = sk.final_pairs(_pair(0, 0, 0, 0), s1, s2)
    assert fin.placed.tolist() == [True, True] and not fin.paired.any() and fin.inv.tolist() == [False, False]
    assert sk.mismatch_lists(GENOME, 0, fin, reads)[2]["placed"] == 2
    assert not sk.final_pairs(_pair(0, 0, 0, 0)).placed.any()
    # a single that is NonUnique places nothing
    assert sk.final_pairs(_pair(0, 0, 0, 0), _single(2, 0, 0), s2).placed.tolist() == [False, True]
    # a NonUnique pair ignores its singles
    assert not sk.final_pairs(_pair(2, 0, 6, 0), s1, s2).placed.any()


def test_sam_text_by_hand():
    g = types.SimpleNamespace(sym=GENOME, frag_start=np.array([0, 6, 10], dtype=np.uint64), frag_names=[" left one", " right"])
    b = _batch([[0, 1, 0, 3], [3, 2, 1, 1], [1, 1, 1, 1]])
    info = np.array([_info(1, 0, errors=1), _info(2, 6, frag=1, errors=1), _info(0, 0)], dtype=np.uint64)
    text, stats = sk.sam_single([g], b, info, np.array([1.5, 2.25, 0], dtype=np.float32), True)
    assert text == ("@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:left\tLN:6\n@SQ\tSN:right\tLN:4\n@PG\tID:real\n"
                    "r0\t0\tleft\t1\t255\t4M\t*\t0\t0\tACAT\t!\"#$\tNM:i:1\tMD:Z:2G1\tZS:f:1.5\n"
                    "r1\t16\tright\t1\t255\t4M\t*\t0\t0\tGGCA\t$#\"!\tNM:i:1\tMD:Z:0T3\tZS:f:2.25\n"
                    "r2\t4\t*\t0\t0\t*\t*\t0\t0\tCCCC\t!\"#$\n")
    assert sk.stderr_line(stats[0], "g.fa") == "sam: file=g.fa placements=2 mismatches=2 on_n=0 disagree=0"
    # a Unique pair in one fragment: flags 1 + 2 + 32 + 64 and 1 + 2 + 16 + 128, TLEN the outer distance with its sign
    b1, b2 = _batch([[0, 1]]), _batch([[3, 1]])                         # AC forward at 0, TC reverse (oriented GA) at 2: text GT
    b1.ids, b2.ids = ["f/1"], ["f/2"]
    text, _ = sk.sam_pairs([g], b1, b2, _pair(1, 0, 2, 0, k2=1), None, None, False, (False, False))
    assert text.split("\n")[4:6] == ["f\t99\tleft\t1\t255\t2M\t=\t3\t4\tAC\t*\tNM:i:0\tMD:Z:2", "f\t147\tleft\t3\t255\t2M\t=\t1\t-4\tGA\t*\tNM:i:1\tMD:Z:1T0"]
    # mate 1 placed on its own, mate 2 not: 1 + 8 + 64 beside 1 + 4 + 128 at its mate's place
    text, _ = sk.sam_pairs([g], b1, b2, _pair(0, 0, 0, 0), _single(1, 0, 0), _single(0, 0, 0), False, (False, False))
    assert text.split("\n")[4:6] == ["f\t73\tleft\t1\t255\t2M\t=\t1\t0\tAC\t*\tNM:i:0\tMD:Z:2", "f\t133\tleft\t1\t0\t*\t=\t1\t0\tTC\t*"]
    # nothing placed: 1 + 4 + 8 + 64 / 128
    text, _ = sk.sam_pairs([g], b1, b2, _pair(2, 0, 2, 0), _single(1, 0, 0), _single(1, 2, 1), False, (False, False))
    assert text.split("\n")[4:6] == ["f\t77\t*\t0\t0\t*\t*\t0\t0\tAC\t*", "f\t141\t*\t0\t0\t*\t*\t0\t0\tTC\t*"]


def test_every_placed_line_of_the_workload_rebuilds_the_genome(ora):
    w = pw.workload()
    letters = "".join("ACGTN"[c] for c in w.g.sym)
    names = {sk.frag_name(n): int(s) for n, s in zip(w.g.frag_names, w.g.frag_start)}
    seen = with_mismatch = 0
    for which in ("main", "long"):
        info, score = pw.oracle_records(ora, which, 1)
        b = getattr(w, which)
        text, stats = sk.sam_single([w.g], b, info, score, True)
        assert stats[0]["disagree"] == 0 and stats[0]["invalid"] == 0
        lines = [l for l in text.split("\n")[:-1] if not l.startswith("@")]
        assert len(lines) == b.n_reads
        for l in lines:
            f = l.split("\t")
            if f[1] == "4":
                assert len(f) == 11
                continue
            assert f[1] in ("0", "16") and f[5] == "%dM" % len(f[9]) and len(f[10]) == len(f[9]) and f[11].startswith("NM:i:") and f[12].startswith("MD:Z:")
            p = names[f[2]] + int(f[3]) - 1
            assert sk.reference_from_md(f[9], f[12][5:]) == letters[p:p + len(f[9])], l
            assert int(f[11][5:]) == sum(c.isalpha() for c in f[12][5:])
            seen += 1
            with_mismatch += f[11] != "NM:i:0"
    assert seen > 1900 and with_mismatch > 1000


# ---- the library and the command line, without a device -------------------------------------------------------------
def test_library_exports_the_mismatch_lists():
    from real_amd import lib as rlib
    L = rlib.load()
    for name in ("real_hip_mismatches", "real_hip_mismatches_pairs", "real_hip_mismatch_stats_get"):
        assert hasattr(L, name) and name in rlib.ABI_SYMBOLS, name
    assert C.sizeof(rlib.RealHipMismatch) == 4 and rlib.MISMATCH_DTYPE.itemsize == 4 and sk.MM_DTYPE == rlib.MISMATCH_DTYPE
    assert C.sizeof(rlib.RealHipMismatchStats) == 8 + 10 * 8
    assert rlib.MISMATCH_STATS_FIELDS[:8] == sk.COUNTERS
    assert L.real_hip_abi_version() == 2
    from real_amd.matcher import HipMatcher
    for name in ("mismatches", "mismatches_pairs", "mismatch_stats"):
        assert callable(getattr(HipMatcher, name))


def test_real_refuses_sam_flags_that_cannot_work(tmp_path):
    """each before anything runs (no device is needed), non-zero, with a message of its own that names the flag"""
    fa, fq, fq2 = str(tmp_path / "g.fa"), str(tmp_path / "r.fq"), str(tmp_path / "r2.fq")
    open(fa, "w").write(">g\nACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT\n")
    for f in (fq, fq2):
        open(f, "w").write("@r\nACGTACGTACGTACGTACGTACGTACGTACGTAC\n+\n" + "I" * 34 + "\n")
    out, sam, other = str(tmp_path / "o.tsv"), str(tmp_path / "o.sam"), str(tmp_path / "x.tsv")
    base = [REAL, "-t", fa, "-p", fq, "-o", out]
    cases = [(base + ["-sam", sam, "-u", "0"], b"-sam writes the unique placement of a read: it cannot be combined with -u 0"),
             (base + ["-p2", fq2, "-sam", sam, "-pairs_all", "1"], b"-sam writes the unique placement of a fragment: it cannot be combined with -pairs_all 1"),
             (base + ["-sam", out], b"-sam must name a file of its own: it names the same file as -o"),
             (base + ["-p2", fq2, "-unpaired", other, "-sam", other], b"same file as -unpaired"),
             (base + ["-p2", fq2, "-insert_hist", other, "-sam", other], b"same file as -insert_hist"),
             (base + ["-pileup", other, "-sam", other], b"same file as -pileup"), (base + ["-pileup_depth", other, "-sam", other], b"same file as -pileup"),
             (base + ["-sam", "-"], b"standard output (-) cannot be it"), (base + ["-sam", ""], b"-sam needs a file name"),
             (base + ["-sam"], b"Parameter for argument -sam is missing")]
    for args, word in cases:
        r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode != 0 and word in r.stderr and b"unknown argument" not in r.stderr, (args, r.stderr.decode()[-600:])
        assert not os.path.exists(sam) and not os.path.exists(other) and not os.path.exists(out)
    r = subprocess.run([REAL, "-h"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    for word in (b"-sam <file", b"SO:unknown", b"NM:i / MD:Z"):
        assert word in r.stderr, word


# ---- the C++ formatter (real_amd/host/Sam.hpp) against the checker, without a device -------------------------------------
SELFTEST = os.path.join(ROOT, "real_amd", "host", "host_selftest")


def _write_refs(d, genomes):
    with open(os.path.join(d, "names.txt"), "w") as f:
        for fi, g in enumerate(genomes):
            for k, name in enumerate(g.frag_names):
                f.write("%d\t%d\t%s\n" % (fi, int(g.frag_start[k]), name))
            f.write("%d\t%d\t\n" % (fi, int(g.frag_start[-1])))


def _write_lists(d, genomes, fin, reads):
    for fi, g in enumerate(genomes):
        L, off, _ = sk.mismatch_lists(g.sym, fi, fin, reads)
        L.tofile(os.path.join(d, "mm%d.bin" % fi))
        off.tofile(os.path.join(d, "moff%d.u64" % fi))


def _selftest(d, fastq, scores, paired):
    r = subprocess.run([SELFTEST, "sam", d, str(int(fastq)), "33", str(int(scores)), str(int(paired))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-1000:]


def _assert_same_text(got, want):
    g, w = got.split("\n"), want.split("\n")
    for k, (a, b) in enumerate(zip(g, w)):
        assert a == b, (k, a, b)
    assert len(g) == len(w)


def test_host_formatter_writes_the_checkers_single_end_file(ora, tmp_path):
    """two genome files, FASTQ and FASTA, scores on and off; the reads as blocks of the host reader and as a chunk of text"""
    from real_amd import synth
    w = pw.workload()
    g2, b2 = pw.second_genome()
    genomes = [w.g, g2]
    reads = synth.concat_batches([w.main, b2])
    info, score = None, None
    for fid, g in enumerate(genomes):
        og = ora.Genome(g.sym, g.frag_start)
        p = ora.make_params(seedl=pw.SEEDL, seedkmax=pw.SEEDK, totalkmax=pw.TOTALK, scores=1, filter_level=pw.FILTER_LEVEL, fileid=fid)
        info, score, _ = ora.match_unique(og, ora.Index(og, pw.SEEDL), p, reads.bases, reads.qual, reads.offsets, info=info, score=score)
    d = str(tmp_path)
    _write_refs(d, genomes)
    info.tofile(os.path.join(d, "info.u64"))
    score.astype(np.float32).tofile(os.path.join(d, "score.f32"))
    _write_lists(d, genomes, sk.final_single(info), sk.single_reads(reads))
    for fastq, scores in ((True, True), (False, False)):
        (synth.reads_to_fastq if fastq else synth.reads_to_fasta)(reads, os.path.join(d, "r1"))
        _selftest(d, fastq, scores, False)
        want, stats = sk.sam_single(genomes, reads, info, score, scores, fastq)
        assert all(st["placed"] > 200 and st["other_file"] > 200 and st["disagree"] == 0 for st in stats)
        for form in ("block.sam", "chunk.sam"):
            _assert_same_text(open(os.path.join(d, form)).read(), want)


def test_host_formatter_writes_the_checkers_paired_file(ora, tmp_path):
    """ragged mates; every flag the checker's records give"""
    import insert_workloads as iw
    import pairs_workloads as pairw
    import singles_checker as sc
    from real_amd import lib as rlib
    from real_amd import synth
    g, b1, b2 = iw.workload("iid", True)
    rec, l1, l2 = iw.records(ora, "iid", True, 1)
    fid, h1, o1, h2, o2 = iw.oracle_lists(ora, "iid", True, 1)
    fm = ora.filter_mult(iw.FILTER_LEVEL, iw.TOTALK)
    s1, s2 = sc.check_singles([(fid, h1, o1)], pairw.lens_of(b1), 1, fm), sc.check_singles([(fid, h2, o2)], pairw.lens_of(b2), 1, fm)
    d = str(tmp_path)
    _write_refs(d, [g])
    pairs = np.zeros(rec.shape[0], dtype=rlib.PAIR_DTYPE)
    for k in rlib.PAIR_DTYPE.names:
        if k != "reserved":
            pairs[k] = rec[k]
    singles = []
    for s in (s1, s2):
        t = np.zeros(s.shape[0], dtype=rlib.SINGLE_DTYPE)
        for k in rlib.SINGLE_DTYPE.names:
            t[k] = s[k]
        singles.append(t)
    pairs.tofile(os.path.join(d, "pairs.bin"))
    singles[0].tofile(os.path.join(d, "s1.bin"))
    singles[1].tofile(os.path.join(d, "s2.bin"))
    _write_lists(d, [g], sk.final_pairs(rec, s1, s2), sk.pair_reads(b1, b2))
    synth.reads_to_fastq(b1, os.path.join(d, "r1"))
    synth.reads_to_fastq(b2, os.path.join(d, "r2"))
    _selftest(d, True, True, True)
    want, stats = sk.sam_pairs([g], b1, b2, rec, s1, s2, True)
    _assert_same_text(open(os.path.join(d, "block.sam")).read(), want)
    flags = set(int(l.split("\t")[1]) for l in want.split("\n")[:-1] if not l.startswith("@"))
    assert {99, 147, 83, 163, 73, 133, 69, 137, 77, 141, 81, 161, 97, 145, 89, 165, 101, 153} <= flags and stats[0]["disagree"] == 0
