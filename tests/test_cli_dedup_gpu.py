"""End-to-end: `real -dedup 1 [-dedup_minq N]`, single-end and with -p2.  Each case runs without the flag, then with it: -o (and
-unpaired) are byte for byte the same; the SAM text is sam_checker's with 1024 added to the FLAG of the marked lines, the pileup
files are pileup_checker's over the records with the duplicates masked, and the `duplicates:` line on standard error is
dup_checker's.  Child processes only, each under its own time limit."""
import re

import numpy as np
import pytest

import dup_checker as dk
import dup_workloads as dw
import insert_workloads as iw
import pileup_checker as pk
import pileup_workloads as pw
import sam_checker as sk
import test_cli_gpu as cli1
import test_cli_pairs_gpu as cli
import test_cli_sam_gpu as clisam
from real_amd import synth

pytestmark = pytest.mark.gpu
MATCH = ["-e", str(pw.TOTALK), "-s", str(pw.SEEDK), "-l", str(pw.SEEDL), "-Q", "33"]


def _both_runs(base, tmp_path, dedup=("-dedup", "1"), unpaired=False):
    """the run without -dedup (-o alone), then with it and -sam / -pileup / -pileup_depth -> (SAM text, pileup file, depth file,
    standard error)"""
    out, plain, sam, pf, df = (str(tmp_path / n) for n in ("out.tsv", "plain.tsv", "out.sam", "pileup.tsv", "depth.tsv"))
    u0, u1 = str(tmp_path / "plain.unpaired"), str(tmp_path / "out.unpaired")
    r0 = cli._run(base + ["-o", plain] + (["-unpaired", u0] if unpaired else []))
    assert r0.returncode == 0, r0.stderr.decode()[-2000:]          # (nothing more is started behind a run that failed)
    r = cli._run(base + ["-o", out, "-sam", sam, "-pileup", pf, "-pileup_depth", df] + list(dedup) + (["-unpaired", u1] if unpaired else []))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out, "rb").read() == open(plain, "rb").read() and len(open(out, "rb").read()) > 10_000
    assert not unpaired or (open(u0, "rb").read() == open(u1, "rb").read() and len(open(u0, "rb").read()) > 1000)
    assert b"duplicates:" not in r0.stderr
    return open(sam).read(), open(pf).read(), open(df).read(), r.stderr.decode()


def _marked_names(b, dup, paired):
    names = {sk.qname(b.ids[i], paired) for i in np.nonzero(dup)[0]}
    assert len(names) == int(dup.sum())                             # (the ids tell the reads apart)
    return names


def _flagged(text):
    return sum(1 for l in text.split("\n") if l and not l.startswith("@") and int(l.split("\t")[1]) & dk.DUP_FLAG)


@pytest.mark.parametrize("extra", [[], ["-batch", "300", "-gpuparse", "0"], ["-chunk", "60000"]])
def test_real_cli_dedup_single_end(ora, tmp_path, extra):
    """one genome file; the reads in one batch, in several batches of the host reader (13 groups span two of them), in several
    chunks of the device parser"""
    dw.assert_single_conditions(ora)
    w = pw.workload()
    fa, rd = cli1.write_inputs(tmp_path, w.g, w.main)
    got, sites, runs, err = _both_runs([cli.REAL, "-t", fa, "-p", rd, "-q", "1"] + MATCH + extra, tmp_path)
    info, score = pw.oracle_records(ora, "main", 1)
    _, sums, dup, st, _ = dw.single_expected(ora, "main")
    plain, _ = sk.sam_single([w.g], w.main, info, score, True)
    clisam._same_text(got, dk.sam_with_marks(plain, _marked_names(w.main, dup, False)))
    assert _flagged(got) == 304 >= 300
    want = dk.pileup_single(w.g.sym, 0, 0, w.main, info, dup)
    assert sites == pk.pileup_lines(want, w.g.frag_start, w.g.frag_names) and runs == pk.depth_lines(want, w.g.frag_start, w.g.frag_names)
    assert (pk.stderr_line(want, fa) + "\n") in err, err[-1500:]
    assert want.stats["placed"] == st["groups"] and want.finish_stats()["max_depth"] < 50          # the hot spot is gone
    assert (dk.stderr_line(st, 15) + "\n") in err, err[-1500:]


def test_real_cli_dedup_two_genome_files(ora, tmp_path):
    """a directory of two genome files: the file id is part of the key, and every file's pileup leaves the duplicates out"""
    w = pw.workload()
    g2, b2 = pw.second_genome()
    by_name = {"a": w.g, "b": g2}
    d = tmp_path / "genomes"
    d.mkdir()
    synth.genome_to_fasta(w.g, str(d / "a.fa"))
    synth.genome_to_fasta(g2, str(d / "b.fa"))
    reads = synth.concat_batches([w.main, b2, b2])                  # (the second file's reads twice: duplicates of file id 1 too)
    reads.ids = reads.ids[:w.main.n_reads + b2.n_reads] + [s + "_again" for s in b2.ids]
    rd = str(tmp_path / "reads.fq")
    synth.reads_to_fastq(reads, rd)
    got, sites, runs, err = _both_runs([cli.REAL, "-t", str(d), "-p", rd, "-batch", "700", "-gpuparse", "0", "-q", "1"] + MATCH, tmp_path)
    order = re.findall(r"Processing file (\S*/([ab])\.fa)", err)         # the file ids follow the directory's own order
    assert sorted(x[1] for x in order) == ["a", "b"]
    order = order[:2]
    info, score = None, None
    for fid, (_, name) in enumerate(order):
        g = by_name[name]
        og = ora.Genome(g.sym, g.frag_start)
        p = ora.make_params(seedl=pw.SEEDL, seedkmax=pw.SEEDK, totalkmax=pw.TOTALK, scores=1, filter_level=pw.FILTER_LEVEL, fileid=fid)
        info, score, _ = ora.match_unique(og, ora.Index(og, pw.SEEDL), p, reads.bases, reads.qual, reads.offsets, info=info, score=score)
    dup, st, groups = dk.mark_single(info, dk.summaries_of(reads, 15))
    assert {k[0] for k, m in groups.items() if len(m) > 1} == {0, 1} and st["duplicates"] > 500
    genomes = [by_name[name] for _, name in order]
    plain, _ = sk.sam_single(genomes, reads, info, score, True)
    clisam._same_text(got, dk.sam_with_marks(plain, _marked_names(reads, dup, False)))
    want_sites, want_runs = "", ""
    for fid, g in enumerate(genomes):
        want = dk.pileup_single(g.sym, fid, 0, reads, info, dup)
        want_sites += pk.pileup_lines(want, g.frag_start, g.frag_names)
        want_runs += pk.depth_lines(want, g.frag_start, g.frag_names)
        assert (pk.stderr_line(want, order[fid][0]) + "\n") in err, err[-1500:]
    assert sites == want_sites and runs == want_runs
    assert (dk.stderr_line(st, 15) + "\n") in err, err[-1500:]


def test_real_cli_dedup_pairs(ora, tmp_path):
    """-p2 on the derived workload: both mates of a duplicate fragment carry 1024, the pileup leaves both out, -unpaired stays"""
    dw.assert_pair_conditions(ora)
    g, b1, b2 = dw.pair_workload()
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-e", str(iw.TOTALK), "-s", "2", "-l", str(iw.SEEDL), "-q", "1", "-batch", "1000"]
    got, sites, runs, err = _both_runs(base, tmp_path, unpaired=True)
    rec, sums1, sums2, dup, st, _ = dw.pair_expected(ora)
    s1, s2 = clisam._singles(dw.pair_lists(ora), b1, b2, 1, ora.filter_mult(iw.FILTER_LEVEL, iw.TOTALK))
    plain, _ = sk.sam_pairs([g], b1, b2, rec, s1, s2, True)
    clisam._same_text(got, dk.sam_with_marks(plain, _marked_names(b1, dup, True)))
    assert _flagged(got) == 2 * 112
    want = dk.pileup_pairs(g.sym, 0, 0, b1, b2, rec, dup)
    assert sites == pk.pileup_lines(want, g.frag_start, g.frag_names) and runs == pk.depth_lines(want, g.frag_start, g.frag_names)
    assert (pk.stderr_line(want, fa) + "\n") in err, err[-1500:]
    assert want.stats["placed"] == 2 * st["groups"]
    assert (dk.stderr_line(st, 15) + "\n") in err, err[-1500:]


def test_real_cli_dedup_minq_changes_the_copy_that_stays(ora, tmp_path):
    """-q 0 (the records do not depend on the qualities) on the main batch with other qualities, chosen with the checker so that
    a group's representative under -dedup_minq 0 is not the default's"""
    w = pw.workload()
    qual = np.random.default_rng(2).integers(0, 41, size=w.main.qual.shape[0]).astype(np.uint8)
    b = synth.ReadBatch(bases=w.main.bases, qual=qual, offsets=w.main.offsets, ids=w.main.ids)
    info, _ = pw.oracle_records(ora, "main", 0)
    marks = {mq: dk.mark_single(info, dk.summaries_of(b, mq)) for mq in (0, 15)}
    assert not np.array_equal(marks[0][0], marks[15][0]) and marks[0][1] == marks[15][1]
    fa, rd = cli1.write_inputs(tmp_path, w.g, b)
    plain, _ = sk.sam_single([w.g], b, info, None, False)
    texts, outs = {}, {}
    for mq, flags in ((15, ["-dedup", "1"]), (0, ["-dedup", "1", "-dedup_minq", "0"])):       # (two runs: the default, then 0)
        out, sam = str(tmp_path / ("out%d.tsv" % mq)), str(tmp_path / ("out%d.sam" % mq))
        r = cli._run([cli.REAL, "-t", fa, "-p", rd, "-q", "0", "-o", out, "-sam", sam] + MATCH + flags)
        assert r.returncode == 0, r.stderr.decode()[-2000:]          # (nothing more is started behind a run that failed)
        texts[mq], outs[mq] = open(sam).read(), open(out, "rb").read()
        clisam._same_text(texts[mq], dk.sam_with_marks(plain, _marked_names(b, marks[mq][0], False)))
        assert (dk.stderr_line(marks[mq][1], mq) + "\n") in r.stderr.decode(), r.stderr.decode()[-1500:]
    assert texts[0] != texts[15] and outs[0] == outs[15] and len(outs[0]) > 10_000
