"""End-to-end: `real -p mates1 -p2 mates2 -gapped g.tsv`.  g.tsv holds one line per mate the gap rescue places uniquely, built here
from the checker's records (gap_checker.py over the pair and single checkers' records of the oracle's lists); -o, -unpaired and
-sam are byte for byte what they are without the flag."""
import re

import pytest

import gap_checker as gc
import gap_workloads as gw
import test_cli_pairs_gpu as cli
from real_amd import synth

pytestmark = pytest.mark.gpu

FLAGS = ["-e", str(gw.TOTALKMAX), "-s", "2", "-l", str(gw.SEEDL), "-q", "0", "-filter_level", "0", "-Q", "33"]


def gapped_lines(rec, s1, s2, genomes, b1, b2):
    lines = []
    for i in range(b1.n_reads):
        r = rec[i]
        if gc.state_of(r["tag"]) != gc.UNIQUE:
            continue
        tm = int(gc.target_of(r["tag"]))
        b, a = (b1, b2)[tm], (s2, s1)[tm][i]
        g, ga = genomes[int(r["fileid"])], genomes[int(a["fileid"])]
        l = int(b.offsets[i + 1]) - int(b.offsets[i])
        lines.append("\t".join([b.ids[i], str(tm + 1), "-" if gc.inverted_of(r["tag"]) else "+", g.frag_names[int(r["frag"])],
                                str(int(r["pos"]) - int(g.frag_start[int(r["frag"])]) + 1), gc.cigar_of(r, l), str(int(r["k"]) + abs(int(r["gap"]))),
                                str(int(r["k"])), str(int(r["cost"])), "*" if int(r["second"]) == gc.NONE else str(int(r["second"])),
                                str(int(a["pos"]) - int(ga.frag_start[int(a["frag"])]) + 1)]))
    return lines


def _summary(ctrs):
    return "gap rescue: eligible=%d placed=%d unique=%d gapped=%d\n" % tuple(sum(c[k] for c in ctrs) for k in ("eligible", "placed", "unique", "gapped"))


@pytest.mark.parametrize("extra,gap,prm", [([], [], None), (["-batch", "100"], ["-gap_max", "16", "-gap_flank", "6", "-gap_margin", "2"],
                                                          gc.Params(16, 6, 4, 6, 1, 4 * gw.TOTALKMAX + 6 + 16, 2))])
def test_real_cli_gapped(ora, tmp_path, extra, gap, prm):
    w = gw.workload(seed=5, prm=prm, max_ins=gw.MAX_INS + (32 if prm else 0))
    g, b1, b2 = w["g"], w["b1"], w["b2"]
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-insert_min", str(w["min_ins"]), "-insert_max", str(w["max_ins"])] + FLAGS + extra
    names = ("out.tsv", "u.tsv", "x.sam")
    plain = [str(tmp_path / ("plain_" + n)) for n in names]
    with_flag = [str(tmp_path / n) for n in names]
    gfile = str(tmp_path / "g.tsv")
    r0 = cli._run(base + ["-o", plain[0], "-unpaired", plain[1], "-sam", plain[2]])
    r = cli._run(base + ["-o", with_flag[0], "-unpaired", with_flag[1], "-sam", with_flag[2], "-gapped", gfile] + gap)
    assert r0.returncode == 0 and r.returncode == 0, r.stderr.decode()[-2000:]
    for a, b in zip(plain, with_flag):
        assert open(a, "rb").read() == open(b, "rb").read(), b                 # nothing else changes with the flag
    pairs, s1, s2, _ = gw.oracle_records(ora, w)
    rec, ctr = gc.check_gap(gc.Text(g.sym, g.frag_start, 0), b1, b2, pairs, s1, s2, w["min_ins"], w["max_ins"], w["prm"])
    want = gapped_lines(rec, s1, s2, [g], b1, b2)
    got = open(gfile).read().split("\n")[:-1]
    assert len(want) >= 60 and got == want
    assert any("D" in l.split("\t")[5] for l in want) and any("I" in l.split("\t")[5] for l in want)
    assert prm is not None or any(l.split("\t")[9] != "*" for l in want)          # (a margin leaves few rivals beside a Unique record)
    assert _summary([ctr]) in r.stderr.decode() and b"gap rescue" not in r0.stderr
    # -gapped alone turns the single records on by itself
    r = cli._run(base + ["-o", with_flag[0], "-gapped", gfile] + gap)
    assert r.returncode == 0 and open(gfile).read().split("\n")[:-1] == want and open(with_flag[0], "rb").read() == open(plain[0], "rb").read()


def test_real_cli_gapped_genome_directory(ora, tmp_path):
    """two genome files: every file's pass places the mates whose anchor lies in it, into one array"""
    wa, wb = gw.workload(seed=1, n=100), gw.workload(seed=2, n=100)
    reads = [[w[k].read(i) for w in (wa, wb) for i in range(w[k].n_reads)] for k in ("b1", "b2")]
    ids = ["f%d" % i for i in range(len(reads[0]))]
    b1, b2 = gw.Batch(reads[0], [x + "/1" for x in ids]), gw.Batch(reads[1], [x + "/2" for x in ids])
    d = tmp_path / "genomes"
    d.mkdir()
    synth.genome_to_fasta(wa["g"], str(d / "a.fa"))
    synth.genome_to_fasta(wb["g"], str(d / "b.fa"))
    p1, p2 = cli._write(tmp_path, b1, b2)
    out, gfile = str(tmp_path / "out.tsv"), str(tmp_path / "g.tsv")
    r = cli._run([cli.REAL, "-t", str(d), "-p", p1, "-p2", p2, "-o", out, "-gapped", gfile, "-insert_min", str(gw.MIN_INS), "-insert_max", str(gw.MAX_INS)] + FLAGS)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    order = re.findall(r"Processing file \S*/([ab])\.fa", r.stderr.decode())     # the file ids follow the directory's own order
    assert sorted(set(order)) == ["a", "b"]
    genomes = [{"a": wa["g"], "b": wb["g"]}[x] for x in order[:2]]
    both = dict(wa, b1=b1, b2=b2)
    files, rec, ctrs = None, None, []
    for fid, g in enumerate(genomes):
        pairs, s1, s2, files = gw.oracle_records(ora, both, g=g, fileid=fid, prev=files)
    for fid, g in enumerate(genomes):
        rec, ctr = gc.check_gap(gc.Text(g.sym, g.frag_start, fid), b1, b2, pairs, s1, s2, gw.MIN_INS, gw.MAX_INS, both["prm"], out=rec)
        ctrs.append(ctr)
    want = gapped_lines(rec, s1, s2, genomes, b1, b2)
    assert open(gfile).read().split("\n")[:-1] == want
    assert all(c["other_file"] >= 20 and c["unique"] >= 20 for c in ctrs) and _summary(ctrs) in r.stderr.decode()


def test_real_cli_gapped_loud_errors(tmp_path):
    g = synth.random_genome(60_000, seed=7)
    b1, b2 = synth.sample_pairs(g, 50, 100, 100, 300, 30, 0.0, 8)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    out, gfile = str(tmp_path / "out.tsv"), str(tmp_path / "g.tsv")
    base = [cli.REAL, "-t", fa, "-o", out, "-Q", "33", "-insert_min", "150", "-insert_max", "420", "-p", p1]
    ok = cli._run(base + ["-p2", p2, "-gapped", gfile])
    assert ok.returncode == 0 and b"gap rescue: eligible=" in ok.stderr
    for args, word in ((["-gapped", gfile], b"-p2"), (["-p2", p2, "-gapped", gfile, "-pairs_all", "1"], b"-pairs_all"),
                       (["-p2", p2, "-gapped", out], b"same file as -o"), (["-p2", p2, "-gapped", gfile, "-gap_max", "0"], b"-gap_max"),
                       (["-p2", p2, "-gapped", gfile, "-gap_max", "17"], b"-gap_max"), (["-p2", p2, "-gap_max", "4"], b"need -gapped"),
                       (["-p2", p2, "-gapped", gfile, "-insert_max", "4097"], b"-insert_max of at most 4096")):
        r = cli._run(base + args)
        assert r.returncode != 0 and word in r.stderr and b"Processing file" not in r.stderr, (args, r.stderr.decode()[-500:])
