"""End-to-end: `real -p mates1 -p2 mates2 -pairs_all 1` against lines built from the checker's enumeration
(pairs_all_checker.py over the oracle's match_all lists): per genome file, for every fragment in read order and every
concordant pair in row-major order of the two hit lists, the 11-column line of mate 1 and then of mate 2; the loud
errors of the flag; and that the unique mode prints what it printed before."""
import os
import re
import subprocess

import numpy as np
import pytest

import pairs_all_checker as pac
import pairs_checker as pc
import pairs_workloads as pw
from real_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "real_amd", "host", "real")


# (the helpers of test_cli_pairs_gpu.py, copied: test files do not import each other)
def _seq(bases, inverted):
    return "".join("ACGTN"[c] for c in (synth.revcomp(bases) if inverted else bases))


def _mate_line(b, i, inverted, score, scores, fragname, pos1, k):
    lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
    return "\t".join([b.ids[i], _seq(b.bases[lo:hi], inverted), ("%g" % float(np.float32(score))) if scores else "", "1", "a", str(hi - lo),
                      "-" if inverted else "+", fragname, str(pos1), "", str(k)])


def expected_lines(rec, genomes, b1, b2, scores):
    """the unique mode's lines (as test_cli_pairs_gpu.py builds them)"""
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


def expected_all_lines(recs, g, b1, b2, scores):
    """the lines of one genome file: two per enumerated pair, in the enumeration's order"""
    lines = []
    for r in recs:
        i = int(r["pair"])
        name, fs = g.frag_names[int(r["frag"])], int(g.frag_start[int(r["frag"])])
        lines.append(_mate_line(b1, i, bool(r["inverted1"]), r["score1"], scores, name, int(r["pos1"]) - fs + 1, int(r["k1"])))
        lines.append(_mate_line(b2, i, not r["inverted1"], r["score2"], scores, name, int(r["pos2"]) - fs + 1, int(r["k2"])))
    return lines


def _write(tmp_path, b1, b2):
    p1, p2 = str(tmp_path / "m1.fq"), str(tmp_path / "m2.fq")
    synth.reads_to_fastq(b1, p1)
    synth.reads_to_fastq(b2, p2)
    return p1, p2


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def _enumerate(ora, g, b1, b2, scores, fileid=0):
    (_, h1, o1, h2, o2), _ = pw.oracle_pairs(ora, g, b1, b2, 32, 3, scores, 2, fileid=fileid)
    return (fileid, h1, o1, h2, o2), pac.enumerate_pairs(h1, o1, pw.lens_of(b1), h2, o2, pw.lens_of(b2), pw.MIN_INS, pw.MAX_INS, fileid)


@pytest.mark.parametrize("scores,extra", [(1, []), (0, ["-batch", "400"])])
def test_real_cli_pairs_all(ora, tmp_path, scores, extra):
    g, b1, b2 = pw.pair_workload("families", True, (100, 80), n=1000)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = _write(tmp_path, b1, b2)
    out = str(tmp_path / "out.tsv")
    base = [REAL, "-t", fa, "-p", p1, "-p2", p2, "-o", out, "-insert_min", str(pw.MIN_INS), "-insert_max", str(pw.MAX_INS),
            "-e", "3", "-s", "2", "-l", "32", "-q", str(scores)] + extra
    r = _run(base + ["-pairs_all", "1"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    f, (recs, off) = _enumerate(ora, g, b1, b2, scores)
    want = expected_all_lines(recs, g, b1, b2, scores)
    got = open(out).read().split("\n")[:-1]
    per = (off[1:] - off[:-1]).astype(np.int64)
    assert len(want) > 1200 and (per >= 2).sum() >= 20 and len(got) == len(want)
    assert got == want
    assert ("concordant pairs: %d" % recs.shape[0]) in r.stderr.decode()
    # the same input without the flag (and with -pairs_all 0) prints what the unique mode printed before
    rec = pc.check_pairs([f], pw.lens_of(b1), pw.lens_of(b2), pw.MIN_INS, pw.MAX_INS, scores, ora.filter_mult(2, 3))
    uniq = expected_lines(rec, [g], b1, b2, scores)
    r = _run(base + ([] if scores else ["-pairs_all", "0"]))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out).read().split("\n")[:-1] == uniq and len(uniq) > 600


def test_real_cli_pairs_all_genome_directory(ora, tmp_path):
    """two genome files: the pairs are printed per file, in the order the files are processed; nothing folds across files,
    so the fragments of a stretch both files hold appear once per file"""
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
    r = _run([REAL, "-t", str(d), "-p", p1, "-p2", p2, "-o", out, "-insert_min", "150", "-insert_max", "420", "-e", "3", "-s", "2", "-l", "32",
              "-pairs_all", "1"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    order = re.findall(r"Processing file \S*/([ab])\.fa", r.stderr.decode())     # the file ids follow the directory's own order
    assert sorted(order) == ["a", "b"]
    want, shared_pairs = [], []
    for fid, x in enumerate(order):
        g = {"a": g0, "b": g1}[x]
        _, (recs, off) = _enumerate(ora, g, b1, b2, 1, fileid=fid)
        want += expected_all_lines(recs, g, b1, b2, 1)
        shared_pairs.append(int(((off[1:] - off[:-1])[-100:] > 0).sum()))
    got = open(out).read().split("\n")[:-1]
    assert got == want and len(want) > 1500
    assert min(shared_pairs) >= 90, shared_pairs


def test_real_cli_pairs_all_loud_errors(tmp_path):
    g = synth.random_genome(60_000, seed=7)
    b1, b2 = synth.sample_pairs(g, 50, 100, 100, 300, 30, 0.0, 8)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = _write(tmp_path, b1, b2)
    out = str(tmp_path / "out.tsv")
    base = [REAL, "-t", fa, "-o", out, "-Q", "33", "-insert_min", "150", "-insert_max", "420"]
    r = _run(base + ["-p", p1, "-p2", p2, "-pairs_all", "1"])
    assert r.returncode == 0 and len(open(out).read().split("\n")) - 1 >= 2 * 45, r.stderr.decode()[-500:]
    for args, word in ((["-p", p1, "-pairs_all", "1"], b"-pairs_all"),
                       (["-p", p1, "-p2", p2, "-pairs_all", "1", "-mate_search", "1"], b"-mate_search"),
                       (["-p", p1, "-p2", p2, "-pairs_all", "1", "-u", "0"], b"-u 0"),
                       (["-p", p1, "-p2", p2, "-pairs_all", "1", "-gpus", "2", "-gpus_share_device", "1"], b"-gpus"),
                       (["-p", p1, "-p2", p2, "-pairs_all", "1", "-block", "20000"], b"more than one index block")):
        r = _run(base + args)
        assert r.returncode != 0 and word in r.stderr, (args[1:], r.stderr.decode()[-500:])


def test_real_cli_pairs_all_150bp_seed_64(ora, tmp_path):
    """2 x 150 bases, 64-base seeds, five mismatches, inserts 200..700, random qualities"""
    import mate_search_workloads as mw
    row = mw.PROTOCOL_ROWS[0]
    assert (row.patl, row.seedl, row.tk, row.min_ins, row.max_ins) == ((150, 150), 64, 5, 200, 700)
    g, b1, b2 = mw.protocol_pair_workload(row, "families")
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = _write(tmp_path, b1, b2)
    out = str(tmp_path / "out.tsv")
    r = _run([REAL, "-l", "64", "-e", "5", "-t", fa, "-p", p1, "-p2", p2, "-o", out, "-insert_min", "200", "-insert_max", "700", "-s", "2", "-q", "1",
              "-Q", "33", "-pairs_all", "1"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    (_, h1, o1, h2, o2), _ = pw.oracle_pairs(ora, g, b1, b2, 64, 5, 1, 2)
    recs, off = pac.enumerate_pairs(h1, o1, pw.lens_of(b1), h2, o2, pw.lens_of(b2), 200, 700, 0)
    want = expected_all_lines(recs, g, b1, b2, 1)
    got = open(out).read().split("\n")[:-1]
    per = (off[1:] - off[:-1]).astype(np.int64)
    assert len(want) > 1200 and (per >= 2).sum() >= 20 and len(got) == len(want)
    assert got == want
    assert ("concordant pairs: %d" % recs.shape[0]) in r.stderr.decode()
