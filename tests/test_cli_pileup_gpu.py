"""End-to-end: `real -pileup <file> -pileup_depth <file> [-pileup_minq Q]`, single-end and with -p2.  The two files and the
summary line on standard error are the checker's (pileup_checker.py over the oracle's final records), and -o is byte for
byte what the run without the flags writes.  Child processes only, each under its own time limit."""
import re

import pytest

import insert_workloads as iw
import pileup_checker as pk
import pileup_workloads as pw
import test_cli_gpu as cli1
import test_cli_pairs_gpu as cli
from real_amd import synth

pytestmark = pytest.mark.gpu
MATCH = ["-e", str(pw.TOTALK), "-s", str(pw.SEEDK), "-l", str(pw.SEEDL), "-q", "1", "-Q", "33"]


def _files(tmp_path):
    return str(tmp_path / "out.tsv"), str(tmp_path / "plain.tsv"), str(tmp_path / "pileup.tsv"), str(tmp_path / "depth.tsv")


def _both_runs(base, out, plain, flags):
    r0 = cli._run(base + ["-o", plain])
    assert r0.returncode == 0, r0.stderr.decode()[-2000:]          # (nothing more is started behind a run that failed)
    r = cli._run(base + ["-o", out] + flags)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out, "rb").read() == open(plain, "rb").read() and len(open(out, "rb").read()) > 10_000
    assert b"pileup:" not in r0.stderr
    return r.stderr.decode()


@pytest.mark.parametrize("extra,min_qual", [([], 0), (["-batch", "300", "-gpuparse", "0"], 0), (["-chunk", "60000"], 0), ([], 20)])
def test_real_cli_pileup_single_end(ora, tmp_path, extra, min_qual):
    """one genome file; the reads in one batch, in several batches of the host reader, in several chunks of the device parser"""
    w = pw.workload()
    fa, rd = cli1.write_inputs(tmp_path, w.g, w.main)
    out, plain, pf, df = _files(tmp_path)
    base = [cli.REAL, "-t", fa, "-p", rd] + MATCH + extra
    err = _both_runs(base, out, plain, ["-pileup", pf, "-pileup_depth", df] + (["-pileup_minq", "20"] if min_qual else []))
    info, score = pw.oracle_records(ora, "main", 1)
    assert open(out).read().split("\n")[:-1] == cli1.expected_unique(ora, w.g, w.main, info, score, 1)
    want = pw.expected(ora, "main", 1, min_qual)
    assert open(pf).read() == pk.pileup_lines(want, w.g.frag_start, w.g.frag_names)
    assert open(df).read() == pk.depth_lines(want, w.g.frag_start, w.g.frag_names)
    assert (pk.stderr_line(want, fa) + "\n") in err, err[-1500:]
    assert want.finish_stats()["sites"] > 100 and want.finish_stats()["max_depth"] >= 300 and (not min_qual or want.stats["low_qual"] > 100)
    assert len(open(df).read().split("\n")) > 1000


def test_real_cli_pileup_two_genome_files(ora, tmp_path):
    """a directory of two genome files: the records fold over both, each file's pileup takes the records of its own file id"""
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
    out, plain, pf, df = _files(tmp_path)
    err = _both_runs([cli.REAL, "-t", str(d), "-p", rd, "-batch", "700", "-gpuparse", "0"] + MATCH, out, plain, ["-pileup", pf, "-pileup_depth", df])
    order = re.findall(r"Processing file (\S*/([ab])\.fa)", err)         # the file ids follow the directory's own order
    assert sorted(x[1] for x in order) == ["a", "b"]
    info, score = None, None
    for fid, (_, name) in enumerate(order):
        g = by_name[name]
        og = ora.Genome(g.sym, g.frag_start)
        p = ora.make_params(seedl=pw.SEEDL, seedkmax=pw.SEEDK, totalkmax=pw.TOTALK, scores=1, filter_level=pw.FILTER_LEVEL, fileid=fid)
        info, score, _ = ora.match_unique(og, ora.Index(og, pw.SEEDL), p, reads.bases, reads.qual, reads.offsets, info=info, score=score)
    sites, runs = "", ""
    for fid, (path, name) in enumerate(order):
        g = by_name[name]
        want = pk.Pileup(g.sym, fid, 0)
        want.add(reads, info)
        assert want.stats["placed"] > 200 and want.stats["other_file"] > 200 and want.finish_stats()["sites"] > 50
        sites += pk.pileup_lines(want, g.frag_start, g.frag_names)
        runs += pk.depth_lines(want, g.frag_start, g.frag_names)
        assert (pk.stderr_line(want, path) + "\n") in err, err[-1500:]
    assert open(pf).read() == sites and open(df).read() == runs


def test_real_cli_pileup_pairs(ora, tmp_path):
    """-p2 with the default paired driver: both mates of every Unique fragment"""
    g, b1, b2 = iw.workload("iid", True)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    out, plain, pf, df = _files(tmp_path)
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-e", str(iw.TOTALK), "-s", "2", "-l", str(iw.SEEDL), "-q", "1", "-batch", "1000"]
    err = _both_runs(base, out, plain, ["-pileup", pf, "-pileup_depth", df])
    rec, l1, l2 = iw.records(ora, "iid", True, 1)
    assert open(out).read().split("\n")[:-1] == cli.expected_lines(rec, [g], b1, b2, 1)
    want = pk.Pileup(g.sym, 0, 0)
    want.add_pairs(b1, b2, rec)
    assert want.stats["placed"] > 2000 and want.finish_stats()["sites"] > 500
    assert open(pf).read() == pk.pileup_lines(want, g.frag_start, g.frag_names)
    assert open(df).read() == pk.depth_lines(want, g.frag_start, g.frag_names)
    assert (pk.stderr_line(want, fa) + "\n") in err, err[-1500:]
