"""End-to-end: `real -p mates1 -p2 mates2 -insert_min A -insert_max B` against lines built from the checker's records
(pairs_checker.py over the oracle's match_all lists): for every Unique fragment the 11-column line of mate 1, then of
mate 2; and the loud errors of the paired-end mode."""
import os
import re
import subprocess

import numpy as np
import pytest

import pairs_checker as pc
import pairs_workloads as pw
from real_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "real_amd", "host", "real")


def _seq(bases, inverted):
    return "".join("ACGTN"[c] for c in (synth.revcomp(bases) if inverted else bases))


def _mate_line(b, i, inverted, score, scores, fragname, pos1, k):
    lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
    return "\t".join([b.ids[i], _seq(b.bases[lo:hi], inverted), ("%g" % float(np.float32(score))) if scores else "", "1", "a", str(hi - lo),
                      "-" if inverted else "+", fragname, str(pos1), "", str(k)])


def expected_lines(rec, genomes, b1, b2, scores):
    lines = []
    for i in range(b1.n_reads):
        r = rec[i]
        if r["state"] != pc.UNIQUE:
            continue
        g = genomes[int(r["fileid"])]
        name, fs = g.frag_names[int(r["frag"])], int(g.frag_start[int(r["frag"])])
        lines.append(_mate_line(b1, i, bool(r["inverted1"]), r["score1"], scores, name, int(r["pos1"]) - fs + 1, int(r["k1"])))
        lines.append(_mate_line(b2, i, not r["inverted1"], r["score2"], scores, name, int(r["pos2"]) - fs + 1, int(r["k2"])))
    return lines


def _write(tmp_path, b1, b2, fastq1=True, fastq2=True):
    p1 = str(tmp_path / ("m1.fq" if fastq1 else "m1.fa"))
    p2 = str(tmp_path / ("m2.fq" if fastq2 else "m2.fa"))
    (synth.reads_to_fastq if fastq1 else synth.reads_to_fasta)(b1, p1)
    (synth.reads_to_fastq if fastq2 else synth.reads_to_fasta)(b2, p2)
    return p1, p2


def _as_fasta(b):
    """what the matcher sees of a FASTA file: constant quality 30"""
    return synth.ReadBatch(bases=b.bases, qual=np.full_like(b.qual, 30), offsets=b.offsets, ids=b.ids)


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


@pytest.mark.parametrize("scores,fastq1,fastq2,extra", [(1, True, True, []), (0, True, True, ["-batch", "400"]), (1, False, False, []),
                                                       (1, True, False, ["-batch", "700"])])
def test_real_cli_pairs(ora, tmp_path, scores, fastq1, fastq2, extra):
    g, b1, b2 = pw.pair_workload("families", True, (100, 80), n=1000)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = _write(tmp_path, b1, b2, fastq1, fastq2)
    out = str(tmp_path / "out.tsv")
    r = _run([REAL, "-t", fa, "-p", p1, "-p2", p2, "-o", out, "-insert_min", str(pw.MIN_INS), "-insert_max", str(pw.MAX_INS),
              "-e", "3", "-s", "2", "-l", "32", "-q", str(scores)] + extra)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    o1, o2 = (b1 if fastq1 else _as_fasta(b1)), (b2 if fastq2 else _as_fasta(b2))
    f, _ = pw.oracle_pairs(ora, g, o1, o2, 32, 3, scores, 2)
    rec = pc.check_pairs([f], pw.lens_of(b1), pw.lens_of(b2), pw.MIN_INS, pw.MAX_INS, scores, ora.filter_mult(2, 3))
    want = expected_lines(rec, [g], b1, b2, scores)
    got = open(out).read().split("\n")[:-1]
    assert len(want) > 600 and len(got) == len(want)
    assert got == want
    assert ("unique fragments: %d" % (len(want) // 2)) in r.stderr.decode()


def test_real_cli_pairs_genome_directory(ora, tmp_path):
    """two genome files fold through the in/out records; fragments of a stretch both files hold print nothing"""
    g0 = synth.random_genome(150_000, seed=501, n_frag=2)
    g1 = synth.random_genome(120_000, seed=502, n_frag=3)
    g1.sym[1000:2600] = g0.sym[1000:2600]
    pa = synth.sample_pairs(g0, 400, 100, 100, 300, 30, 0.01, 61, insert_min=150, insert_max=420)
    pb = synth.sample_pairs(g1, 300, 100, 100, 300, 30, 0.01, 62, insert_min=150, insert_max=420)
    shared = synth.Genome(sym=g0.sym[1000:2600].copy(), frag_start=np.array([0, 1600], dtype=np.uint64))
    ps = synth.sample_pairs(shared, 100, 100, 100, 300, 30, 0.0, 63, insert_min=150, insert_max=420, straddle_frac=0)
    b1 = synth.concat_batches([pa[0], pb[0], ps[0]])
    b2 = synth.concat_batches([pa[1], pb[1], ps[1]])
    d = tmp_path / "genomes"
    d.mkdir()
    synth.genome_to_fasta(g0, str(d / "a.fa"))
    synth.genome_to_fasta(g1, str(d / "b.fa"))
    p1, p2 = _write(tmp_path, b1, b2)
    out = str(tmp_path / "out.tsv")
    r = _run([REAL, "-t", str(d), "-p", p1, "-p2", p2, "-o", out, "-insert_min", "150", "-insert_max", "420", "-e", "3", "-s", "2", "-l", "32"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    order = re.findall(r"Processing file \S*/([ab])\.fa", r.stderr.decode())     # the file ids follow the directory's own order
    assert sorted(order) == ["a", "b"]
    genomes = [{"a": g0, "b": g1}[x] for x in order]
    files = [pw.oracle_pairs(ora, g, b1, b2, 32, 3, 1, 2, fileid=fid)[0] for fid, g in enumerate(genomes)]
    rec = pc.check_pairs(files, pw.lens_of(b1), pw.lens_of(b2), 150, 420, 1, ora.filter_mult(2, 3))
    want = expected_lines(rec, genomes, b1, b2, 1)
    got = open(out).read().split("\n")[:-1]
    assert got == want and len(want) > 1000
    assert (rec["state"][-100:] == pc.NONUNIQUE).sum() >= 90


def test_real_cli_pairs_loud_errors(tmp_path):
    g = synth.random_genome(60_000, seed=7)
    b1, b2 = synth.sample_pairs(g, 50, 100, 100, 300, 30, 0.0, 8)
    b3, _ = synth.sample_pairs(g, 49, 100, 100, 300, 30, 0.0, 8)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = _write(tmp_path, b1, b2)
    p3 = str(tmp_path / "short.fq")
    synth.reads_to_fastq(b3, p3)
    out = str(tmp_path / "out.tsv")
    base = [REAL, "-t", fa, "-o", out, "-Q", "33", "-insert_min", "150", "-insert_max", "420"]     # (error-free reads: one quality character, no detection)
    assert _run(base + ["-p", p1, "-p2", p2]).returncode == 0
    for args, word in ((["-p", p1, "-p2", p3], b"different numbers of reads"), (["-p", p3, "-p2", p2], b"different numbers of reads"),
                       (["-p", p1, "-p2", p2, "-u", "0"], b"-u 0"), (["-p", p1, "-p2", p2, "-gpus", "2", "-gpus_share_device", "1"], b"-gpus"),
                       (["-p", p1, "-p2", p2, "-block", "20000"], b"more than one index block"),
                       (["-p", p1, "-p2", p2, "-insert_min", "500"], b"-insert_min")):
        r = _run(base + args)
        assert r.returncode != 0 and word in r.stderr, (args[3:], r.stderr.decode()[-500:])
