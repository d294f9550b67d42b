"""End-to-end: `real -vcf <file> [-vcf_minqual Q] [-vcf_mindepth D]`, single-end and with -p2, with and without -pileup and
-dedup 1.  The VCF and the summary line on standard error are the checker's (call_checker.py over the oracle's final records),
and -o is byte for byte what the run without the flags writes.  Child processes only, each under its own time limit."""
import functools
import os
import re

import numpy as np
import pytest

import call_checker as ck
import call_workloads as cw
import dup_checker as dk
import dup_workloads as dw
import insert_workloads as iw
import pileup_checker as pk
import pileup_workloads as pw
import test_cli_gpu as cli1
import test_cli_pairs_gpu as cli
from real_amd import synth

pytestmark = pytest.mark.gpu
MATCH = ["-e", str(cw.TOTALK), "-s", str(cw.SEEDK), "-l", str(cw.SEEDL), "-q", "1", "-Q", "33"]
COV_SLICE = 4000                       # reads of the 40x batch that go through the command line (the whole of it goes through the library)


@functools.lru_cache(maxsize=None)
def _reads():
    """the ragged batch with its hot spot, the long reads and a tenth of the 40x batch as one read file"""
    w = cw.workload()
    head = synth.ReadBatch(bases=w.cov.bases[:COV_SLICE * cw.COV_LEN], qual=w.cov.qual[:COV_SLICE * cw.COV_LEN], offsets=w.cov.offsets[:COV_SLICE + 1],
                           ids=w.cov.ids[:COV_SLICE])
    return synth.concat_batches([w.ragged, w.long, head])


def _records(ora):
    return np.concatenate([cw.oracle_records(ora, "ragged"), cw.oracle_records(ora, "long"), cw.oracle_records(ora, "cov")[:COV_SLICE]])


_want = {}


def _expected(ora, min_qual):
    if min_qual not in _want:
        pu = pk.Pileup(cw.workload().g.sym, 0, min_qual)
        pu.add(_reads(), _records(ora))
        cl = ck.Calls(pu)
        cl.add(_reads(), _records(ora))
        _want[min_qual] = (pu, cl)
    return _want[min_qual]


def _names(g):
    return [s.split()[0] for s in g.frag_names]                   # what -sam's @SQ lines carry


def _contigs(genomes):
    return [(name, int(g.frag_start[k + 1] - g.frag_start[k])) for g in genomes for k, name in enumerate(_names(g))]


def _both_runs(base, tmp_path, flags):
    """the run with -o alone, then with the flags -> standard error of the second; -o byte for byte the same"""
    out, plain = str(tmp_path / "out.tsv"), str(tmp_path / "plain.tsv")
    r0 = cli._run(base + ["-o", plain])
    assert r0.returncode == 0, r0.stderr.decode()[-2000:]          # (nothing more is started behind a run that failed)
    r = cli._run(base + ["-o", out] + flags)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out, "rb").read() == open(plain, "rb").read() and len(open(out, "rb").read()) > 10_000
    assert b"calls:" not in r0.stderr and b"pileup:" not in r0.stderr
    return r.stderr.decode()


@pytest.mark.parametrize("extra,min_qual", [([], 20), (["-batch", "300", "-gpuparse", "0"], 0), (["-chunk", "60000"], 20)])
def test_real_cli_vcf_single_end(ora, tmp_path, extra, min_qual):
    """one genome file; the reads in one batch, in several batches of the host reader, in several chunks of the device parser;
    -vcf beside -pileup"""
    w = cw.workload()
    fa, rd = cli1.write_inputs(tmp_path, w.g, _reads())
    vf, pf = str(tmp_path / "calls.vcf"), str(tmp_path / "pileup.tsv")
    err = _both_runs([cli.REAL, "-t", fa, "-p", rd] + MATCH + extra, tmp_path, ["-vcf", vf, "-pileup", pf] + (["-pileup_minq", "20"] if min_qual else []))
    pu, cl = _expected(ora, min_qual)
    calls = cl.calls()
    assert calls.shape[0] > 60 and (calls["a1"] != calls["a2"]).sum() > 20 and (calls["a1"] == calls["a2"]).sum() > 20
    assert open(vf).read() == ck.vcf_header(_contigs([w.g])) + ck.vcf_lines(calls, w.g.frag_start, _names(w.g))
    assert open(pf).read() == pk.pileup_lines(pu, w.g.frag_start, w.g.frag_names)
    assert (pk.stderr_line(pu, fa) + "\n") in err and (ck.stderr_line(cl, fa) + "\n") in err, err[-1500:]


def test_real_cli_vcf_without_pileup_and_with_thresholds(ora, tmp_path):
    """-vcf alone runs the pileup without writing a sites file, and -pileup_minq applies to it"""
    w = cw.workload()
    fa, rd = cli1.write_inputs(tmp_path, w.g, _reads())
    vf = str(tmp_path / "calls.vcf")
    err = _both_runs([cli.REAL, "-t", fa, "-p", rd] + MATCH, tmp_path, ["-vcf", vf, "-pileup_minq", "20", "-vcf_minqual", "60", "-vcf_mindepth", "9"])
    pu, cl = _expected(ora, 20)
    calls = cl.calls(60, 9)
    assert 20 < calls.shape[0] < cl.calls().shape[0]
    assert open(vf).read() == ck.vcf_header(_contigs([w.g])) + ck.vcf_lines(calls, w.g.frag_start, _names(w.g))
    assert (ck.stderr_line(cl, fa, 60, 9) + "\n") in err and (pk.stderr_line(pu, fa) + "\n") in err, err[-1500:]
    assert sorted(os.listdir(str(tmp_path))) == sorted(["calls.vcf", "out.tsv", "plain.tsv", os.path.basename(fa), os.path.basename(rd)])


def test_real_cli_vcf_two_genome_files(ora, tmp_path):
    """a directory of two genome files: one header with the fragments of both, each file's calls from the records of its own file id"""
    w = cw.workload()
    g2, b2 = pw.second_genome()
    by_name = {"a": w.g, "b": g2}
    d = tmp_path / "genomes"
    d.mkdir()
    synth.genome_to_fasta(w.g, str(d / "a.fa"))
    synth.genome_to_fasta(g2, str(d / "b.fa"))
    reads = synth.concat_batches([_reads(), b2])
    rd = str(tmp_path / "reads.fq")
    synth.reads_to_fastq(reads, rd)
    vf = str(tmp_path / "calls.vcf")
    err = _both_runs([cli.REAL, "-t", str(d), "-p", rd, "-batch", "700", "-gpuparse", "0"] + MATCH, tmp_path, ["-vcf", vf, "-vcf_minqual", "10", "-vcf_mindepth", "2"])
    order = re.findall(r"Processing file (\S*/([ab])\.fa)", err)         # the file ids follow the directory's own order
    assert sorted(x[1] for x in order) == ["a", "b"]
    info, score = None, None
    for fid, (_, name) in enumerate(order):
        g = by_name[name]
        og = ora.Genome(g.sym, g.frag_start)
        p = ora.make_params(seedl=cw.SEEDL, seedkmax=cw.SEEDK, totalkmax=cw.TOTALK, scores=1, filter_level=cw.FILTER_LEVEL, fileid=fid)
        info, score, _ = ora.match_unique(og, ora.Index(og, cw.SEEDL), p, reads.bases, reads.qual, reads.offsets, info=info, score=score)
    text = ck.vcf_header(_contigs([by_name[name] for _, name in order]))
    for fid, (path, name) in enumerate(order):
        g = by_name[name]
        pu = pk.Pileup(g.sym, fid, 0)
        pu.add(reads, info)
        cl = ck.Calls(pu)
        cl.add(reads, info)
        assert cl.stats["placed"] > 200 and cl.stats["other_file"] > 200 and cl.calls(10, 2).shape[0] > (50 if name == "a" else 0)
        text += ck.vcf_lines(cl.calls(10, 2), g.frag_start, _names(g))
        assert (ck.stderr_line(cl, path, 10, 2) + "\n") in err, err[-1500:]
    assert open(vf).read() == text


def test_real_cli_vcf_pairs(ora, tmp_path):
    """-p2 with the default paired driver on the duplicate workload's pairs: the evidence of both mates of every Unique fragment"""
    g, b1, b2 = dw.pair_workload()
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    vf = str(tmp_path / "calls.vcf")
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-e", str(iw.TOTALK), "-s", "2", "-l", str(iw.SEEDL), "-q", "1", "-batch", "1000"]
    err = _both_runs(base, tmp_path, ["-vcf", vf, "-pileup_minq", "10", "-vcf_minqual", "0", "-vcf_mindepth", "1"])
    rec = dw.pair_expected(ora)[0]
    pu = pk.Pileup(g.sym, 0, 10)
    pu.add_pairs(b1, b2, rec)
    cl = ck.Calls(pu)
    cl.add_pairs(b1, b2, rec)
    calls = cl.calls(0, 1)
    assert cl.stats["placed"] > 2000 and cl.site_list.shape[0] > 50 and cl.stats["low_qual"] > 100 and calls.shape[0] > 20
    assert open(vf).read() == ck.vcf_header(_contigs([g])) + ck.vcf_lines(calls, g.frag_start, _names(g))
    assert (ck.stderr_line(cl, fa, 0, 1) + "\n") in err, err[-1500:]


def test_real_cli_vcf_dedup(ora, tmp_path):
    """-dedup 1: the duplicates are gone from the pileup and from the evidence (the 300-copy hot spot counts once per strand)"""
    dw.assert_single_conditions(ora)
    w = pw.workload()
    fa, rd = cli1.write_inputs(tmp_path, w.g, w.main)
    vf = str(tmp_path / "calls.vcf")
    flags = ["-vcf", vf, "-vcf_minqual", "0", "-vcf_mindepth", "1"]
    err = _both_runs([cli.REAL, "-t", fa, "-p", rd] + MATCH, tmp_path, flags + ["-dedup", "1"])
    info, _ = pw.oracle_records(ora, "main", 1)
    _, _, dup, st, _ = dw.single_expected(ora, "main")
    masked = dk.masked_info(info, dup)
    pu = dk.pileup_single(w.g.sym, 0, 0, w.main, info, dup)
    cl = ck.Calls(pu)
    cl.add(w.main, masked)
    assert cl.stats["placed"] == st["groups"] and int(cl.cnt.sum(axis=1).max()) < 50 and cl.calls(0, 1).shape[0] > 20
    assert open(vf).read() == ck.vcf_header(_contigs([w.g])) + ck.vcf_lines(cl.calls(0, 1), w.g.frag_start, _names(w.g))
    assert (ck.stderr_line(cl, fa, 0, 1) + "\n") in err, err[-1500:]
    full = ck.Calls(pw.expected(ora, "main", 1, 0))                     # (without -dedup the hot spot would be in the evidence)
    full.add(w.main, info)
    assert int(full.cnt.sum(axis=1).max()) >= 300
