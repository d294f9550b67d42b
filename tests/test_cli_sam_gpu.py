"""End-to-end: `real -sam <file>`, single-end and with -p2.  The SAM file is byte for byte the checker's (sam_checker.py over
the oracle's final records and the pair / single checkers'), the summary line of every genome file on standard error is the
checker's, and -o is byte for byte what the run without the flag writes.  Child processes only, each under its own time limit."""
import re

import pytest

import insert_workloads as iw
import mate_search_checker as mc
import mate_search_workloads as mw
import pairs_checker as pc
import pairs_workloads as pairw
import pileup_workloads as pw
import sam_checker as sk
import singles_checker as sc
import test_cli_gpu as cli1
import test_cli_pairs_gpu as cli
from real_amd import synth

pytestmark = pytest.mark.gpu
MATCH = ["-e", str(pw.TOTALK), "-s", str(pw.SEEDK), "-l", str(pw.SEEDL), "-q", "1", "-Q", "33"]


def _both_runs(base, tmp_path):
    """the run without -sam, then with it: -o does not change -> (the SAM text, standard error of the second run)"""
    out, plain, sam = str(tmp_path / "out.tsv"), str(tmp_path / "plain.tsv"), str(tmp_path / "out.sam")
    r0 = cli._run(base + ["-o", plain])
    assert r0.returncode == 0, r0.stderr.decode()[-2000:]          # (nothing more is started behind a run that failed)
    r = cli._run(base + ["-o", out, "-sam", sam])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out, "rb").read() == open(plain, "rb").read() and len(open(out, "rb").read()) > 10_000
    assert b"sam:" not in r0.stderr
    return open(sam).read(), r.stderr.decode(), open(out).read()


def _same_text(got, want):
    g, w = got.split("\n"), want.split("\n")
    for k, (a, b) in enumerate(zip(g, w)):
        assert a == b, (k, a, b)
    assert len(g) == len(w)


def _check_stderr(err, stats, paths):
    for st, path in zip(stats, paths):
        assert st["disagree"] == 0
        assert (sk.stderr_line(st, path) + "\n") in err, err[-1500:]


@pytest.mark.parametrize("extra", [[], ["-batch", "300", "-gpuparse", "0"], ["-chunk", "60000"]])
def test_real_cli_sam_single_end(ora, tmp_path, extra):
    """one genome file; the reads in one batch, in several batches of the host reader, in several chunks of the device parser"""
    w = pw.workload()
    fa, rd = cli1.write_inputs(tmp_path, w.g, w.main)
    got, err, out = _both_runs([cli.REAL, "-t", fa, "-p", rd] + MATCH + extra, tmp_path)
    info, score = pw.oracle_records(ora, "main", 1)
    assert out.split("\n")[:-1] == cli1.expected_unique(ora, w.g, w.main, info, score, 1)
    want, stats = sk.sam_single([w.g], w.main, info, score, True)
    _same_text(got, want)
    _check_stderr(err, stats, [fa])
    assert stats[0]["placed"] > 1500 and stats[0]["mismatches"] > 3000 and want.count("\t4\t*\t0\t0\t*\t") > 50


def test_real_cli_sam_fasta_and_no_scores(ora, tmp_path):
    """FASTA reads: QUAL is *; -q 0: no ZS tag"""
    w = pw.workload()
    fa, rd = cli1.write_inputs(tmp_path, w.g, w.main, fastq=False)
    base = [cli.REAL, "-t", fa, "-p", rd, "-e", str(pw.TOTALK), "-s", str(pw.SEEDK), "-l", str(pw.SEEDL), "-q", "0"]
    got, err, _ = _both_runs(base, tmp_path)
    info, _ = pw.oracle_records(ora, "main", 0)          # (without scores the qualities play no part)
    want, stats = sk.sam_single([w.g], w.main, info, None, False, fastq=False)
    _same_text(got, want)
    _check_stderr(err, stats, [fa])
    assert "ZS:f:" not in got and "\t*\tNM:i:" in got


def test_real_cli_sam_two_genome_files(ora, tmp_path):
    """a directory of two genome files: each file's pass writes the reads placed in it, the last one those placed nowhere"""
    w = pw.workload()
    g2, b2 = pw.second_genome()
    by_name = {"a": w.g, "b": g2}
    d = tmp_path / "genomes"
    d.mkdir()
    synth.genome_to_fasta(w.g, str(d / "a.fa"))
    synth.genome_to_fasta(g2, str(d / "b.fa"))
    reads = synth.concat_batches([w.main, b2])
    rd = str(tmp_path / "reads.fq")
    synth.reads_to_fastq(reads, rd)
    got, err, _ = _both_runs([cli.REAL, "-t", str(d), "-p", rd, "-batch", "700", "-gpuparse", "0"] + MATCH, tmp_path)
    order = re.findall(r"Processing file (\S*/([ab])\.fa)", err)         # the file ids follow the directory's own order
    assert sorted(x[1] for x in order) == ["a", "b"]
    info, score = None, None
    for fid, (_, name) in enumerate(order):
        g = by_name[name]
        og = ora.Genome(g.sym, g.frag_start)
        p = ora.make_params(seedl=pw.SEEDL, seedkmax=pw.SEEDK, totalkmax=pw.TOTALK, scores=1, filter_level=pw.FILTER_LEVEL, fileid=fid)
        info, score, _ = ora.match_unique(og, ora.Index(og, pw.SEEDL), p, reads.bases, reads.qual, reads.offsets, info=info, score=score)
    want, stats = sk.sam_single([by_name[name] for _, name in order], reads, info, score, True)
    _same_text(got, want)
    _check_stderr(err, stats, [path for path, _ in order])
    assert all(st["placed"] > 200 and st["other_file"] > 200 for st in stats) and want.count("@SQ") == 5


def _singles(f, b1, b2, scores, fm):
    fid, h1, o1, h2, o2 = f
    return (sc.check_singles([(fid, h1, o1)], pairw.lens_of(b1), scores, fm), sc.check_singles([(fid, h2, o2)], pairw.lens_of(b2), scores, fm))


def test_real_cli_sam_pairs_of_differing_lengths(ora, tmp_path):
    """-p2 with the default paired driver on ragged mates (100 / 80 and 60 / 120 bases): the pair flags, RNEXT / PNEXT, TLEN"""
    g, b1, b2 = iw.workload("iid", True)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-e", str(iw.TOTALK), "-s", "2", "-l", str(iw.SEEDL), "-q", "1", "-batch", "1000"]
    got, err, out = _both_runs(base, tmp_path)
    rec, l1, l2 = iw.records(ora, "iid", True, 1)
    assert out.split("\n")[:-1] == cli.expected_lines(rec, [g], b1, b2, 1)
    s1, s2 = _singles(iw.oracle_lists(ora, "iid", True, 1), b1, b2, 1, ora.filter_mult(iw.FILTER_LEVEL, iw.TOTALK))
    want, stats = sk.sam_pairs([g], b1, b2, rec, s1, s2, True)
    _same_text(got, want)
    _check_stderr(err, stats, [fa])
    flags = [int(l.split("\t")[1]) for l in want.split("\n")[:-1] if not l.startswith("@")]
    assert len(flags) == 2 * b1.n_reads and (l1 != l2).sum() > 500
    for f, floor in ((99, 300), (147, 300), (83, 300), (163, 300), (73, 20), (133, 20), (69, 20), (137, 20), (77, 100), (141, 100), (81, 10), (161, 10)):
        assert flags.count(f) >= floor, (f, flags.count(f))
    assert any(f & 12 == 0 and f & 2 == 0 for f in flags)      # both mates placed on their own, not as a pair


def test_real_cli_sam_pairs_with_the_mate_search(ora, tmp_path):
    """-mate_search 1: the pair records are final after the search, the singles stay folds of seed hits"""
    g, b1, b2, planted = mw.search_workload("families", True, (100, 80), 32, 3)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-insert_min", str(mw.MIN_INS), "-insert_max", str(mw.MAX_INS), "-e", "3", "-s", "2", "-l", "32",
            "-q", "1", "-mate_search", "1"]
    got, err, _ = _both_runs(base, tmp_path)
    f = mw.oracle_lists(ora, g, b1, b2, 32, 3, 1, 2)
    fm = ora.filter_mult(2, 3)
    on, _ = mc.check_pairs_search(ora, {0: g}, [f], b1, b2, mw.MIN_INS, mw.MAX_INS, 1, fm, 32, 3)
    s1, s2 = _singles(f, b1, b2, 1, fm)
    want, stats = sk.sam_pairs([g], b1, b2, on, s1, s2, True)
    _same_text(got, want)
    _check_stderr(err, stats, [fa])
    assert int((on["state"] == pc.UNIQUE).sum()) * 2 <= stats[0]["placed"]


def test_real_cli_sam_leaves_every_other_output_alone(tmp_path):
    """-unpaired, -insert_hist, -pileup and -pileup_depth beside -sam: each file is byte for byte what the run without -sam writes"""
    g, b1, b2 = iw.workload("iid", True)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-e", str(iw.TOTALK), "-s", "2", "-l", str(iw.SEEDL), "-q", "1", "-batch", "1000"]
    names = ("-o", "-unpaired", "-insert_hist", "-pileup", "-pileup_depth")
    runs = {}
    for tag, extra in (("off", []), ("on", ["-sam", str(tmp_path / "on.sam")])):
        flags = []
        for k in names:
            flags += [k, str(tmp_path / (tag + k + ".out"))]
        r = cli._run(base + flags + extra)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        runs[tag] = [open(str(tmp_path / (tag + k + ".out")), "rb").read() for k in names]
    for k, a, b in zip(names, runs["off"], runs["on"]):
        assert a == b and len(a) > 100, k
    assert open(str(tmp_path / "on.sam")).read().startswith("@HD\tVN:1.6\tSO:unknown\n@SQ\t")
