"""End-to-end: `real -p mates1 -p2 mates2 -unpaired u.tsv`.  The main output is what it is without the flag, byte for
byte; u.tsv holds, for every fragment whose final pair state is NoMatch, the 11-column line of mate 1 if it is Unique on its
own and then of mate 2 likewise, built here from the checkers' records (pairs_checker.py / singles_checker.py over the
oracle's match_all lists)."""
import re

import numpy as np
import pytest

import mate_search_checker as mc
import mate_search_workloads as mw
import pairs_checker as pc
import pairs_workloads as pw
import singles_checker as sc
import test_cli_pairs_gpu as cli
from real_amd import synth

pytestmark = pytest.mark.gpu


def unpaired_lines(pair_rec, s1, s2, genomes, b1, b2, scores):
    lines = []
    for i in range(b1.n_reads):
        if pair_rec["state"][i] != pc.NOMATCH:
            continue
        for b, s in ((b1, s1[i]), (b2, s2[i])):
            if sc.state_of(s["tag"]) != sc.UNIQUE:
                continue
            g = genomes[int(s["fileid"])]
            name, fs = g.frag_names[int(s["frag"])], int(g.frag_start[int(s["frag"])])
            lines.append(cli._mate_line(b, i, bool(sc.inverted_of(s["tag"])), s["score"], scores, name, int(s["pos"]) - fs + 1, int(sc.k_of(s["tag"]))))
    return lines


def _singles(files, b1, b2, scores, fm):
    s1 = sc.check_singles([(fid, h1, o1) for fid, h1, o1, _, _ in files], pw.lens_of(b1), scores, fm)
    s2 = sc.check_singles([(fid, h2, o2) for fid, _, _, h2, o2 in files], pw.lens_of(b2), scores, fm)
    return s1, s2


@pytest.mark.parametrize("scores,fastq1,fastq2,extra", [(1, True, True, []), (0, True, True, ["-batch", "400"]), (1, False, False, []),
                                                       (1, True, False, ["-batch", "700"])])
def test_real_cli_unpaired(ora, tmp_path, scores, fastq1, fastq2, extra):
    g, b1, b2 = pw.pair_workload("families", True, (100, 80), n=1000)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2, fastq1, fastq2)
    out, plain, u = str(tmp_path / "out.tsv"), str(tmp_path / "plain.tsv"), str(tmp_path / "u.tsv")
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-insert_min", str(pw.MIN_INS), "-insert_max", str(pw.MAX_INS),
            "-e", "3", "-s", "2", "-l", "32", "-q", str(scores)] + extra
    r0 = cli._run(base + ["-o", plain])
    r = cli._run(base + ["-o", out, "-unpaired", u])
    assert r0.returncode == 0 and r.returncode == 0, r.stderr.decode()[-2000:]
    o1, o2 = (b1 if fastq1 else cli._as_fasta(b1)), (b2 if fastq2 else cli._as_fasta(b2))
    f, _ = pw.oracle_pairs(ora, g, o1, o2, 32, 3, scores, 2)
    fm = ora.filter_mult(2, 3)
    rec = pc.check_pairs([f], pw.lens_of(b1), pw.lens_of(b2), pw.MIN_INS, pw.MAX_INS, scores, fm)
    s1, s2 = _singles([f], b1, b2, scores, fm)
    want = cli.expected_lines(rec, [g], b1, b2, scores)
    got = open(out).read().split("\n")[:-1]
    assert len(want) > 600 and got == want
    assert open(out, "rb").read() == open(plain, "rb").read()                  # the main output does not change with the flag
    want_u = unpaired_lines(rec, s1, s2, [g], b1, b2, scores)
    got_u = open(u).read().split("\n")[:-1]
    assert len(want_u) > 50 and len(got_u) == len(want_u)
    assert got_u == want_u
    assert ("unpaired mates: %d\n" % len(want_u)) in r.stderr.decode()
    assert b"unpaired mates" not in r0.stderr


def test_real_cli_unpaired_genome_directory(ora, tmp_path):
    """two genome files fold through the file id: mates of a stretch both files hold are NonUnique and print nothing"""
    g0 = synth.random_genome(150_000, seed=501, n_frag=2)
    g1 = synth.random_genome(120_000, seed=502, n_frag=3)
    g1.sym[1000:2600] = g0.sym[1000:2600]
    pa = synth.sample_pairs(g0, 400, 100, 100, 300, 30, 0.02, 61, insert_min=150, insert_max=420)
    pb = synth.sample_pairs(g1, 300, 100, 100, 300, 30, 0.02, 62, insert_min=150, insert_max=420)
    shared = synth.Genome(sym=g0.sym[1000:2600].copy(), frag_start=np.array([0, 1600], dtype=np.uint64))
    ps = synth.sample_pairs(shared, 100, 100, 100, 300, 30, 0.0, 63, insert_min=150, insert_max=420, straddle_frac=0)
    # discordant fragments: mate 1 of a fragment of the first file with mate 2 of a fragment of the second
    px = (synth.sample_pairs(g0, 60, 100, 100, 300, 30, 0.0, 64, insert_min=150, insert_max=420)[0],
          synth.sample_pairs(g1, 60, 100, 100, 300, 30, 0.0, 65, insert_min=150, insert_max=420)[1])
    b1 = synth.concat_batches([pa[0], pb[0], ps[0], px[0]])
    b2 = synth.concat_batches([pa[1], pb[1], ps[1], px[1]])
    d = tmp_path / "genomes"
    d.mkdir()
    synth.genome_to_fasta(g0, str(d / "a.fa"))
    synth.genome_to_fasta(g1, str(d / "b.fa"))
    p1, p2 = cli._write(tmp_path, b1, b2)
    out, u = str(tmp_path / "out.tsv"), str(tmp_path / "u.tsv")
    r = cli._run([cli.REAL, "-t", str(d), "-p", p1, "-p2", p2, "-o", out, "-unpaired", u, "-insert_min", "150", "-insert_max", "420",
                  "-e", "3", "-s", "2", "-l", "32"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    order = re.findall(r"Processing file \S*/([ab])\.fa", r.stderr.decode())     # the file ids follow the directory's own order
    assert sorted(order) == ["a", "b"]
    genomes = [{"a": g0, "b": g1}[x] for x in order]
    files = [pw.oracle_pairs(ora, g, b1, b2, 32, 3, 1, 2, fileid=fid)[0] for fid, g in enumerate(genomes)]
    fm = ora.filter_mult(2, 3)
    rec = pc.check_pairs(files, pw.lens_of(b1), pw.lens_of(b2), 150, 420, 1, fm)
    s1, s2 = _singles(files, b1, b2, 1, fm)
    assert open(out).read().split("\n")[:-1] == cli.expected_lines(rec, genomes, b1, b2, 1)
    want_u = unpaired_lines(rec, s1, s2, genomes, b1, b2, 1)
    assert open(u).read().split("\n")[:-1] == want_u
    # the mates of the shared stretch are NonUnique through the file id alone; the discordant fragments print both mates,
    # each from its own file
    sh = slice(700, 800)
    assert (sc.state_of(s1["tag"][sh]) == sc.NONUNIQUE).sum() >= 90 and (sc.state_of(s2["tag"][sh]) == sc.NONUNIQUE).sum() >= 90
    ids = set(l.split("\t")[0] for l in want_u)
    assert not any(b1.ids[i] in ids or b2.ids[i] in ids for i in range(700, 800))
    x = slice(800, 860)
    both = (rec["state"][x] == pc.NOMATCH) & (sc.state_of(s1["tag"][x]) == sc.UNIQUE) & (sc.state_of(s2["tag"][x]) == sc.UNIQUE)
    assert both.sum() >= 50 and (s1["fileid"][x][both] != s2["fileid"][x][both]).all()
    assert ("unpaired mates: %d\n" % len(want_u)) in r.stderr.decode() and len(want_u) > 100


def test_real_cli_unpaired_with_the_mate_search(ora, tmp_path):
    """the pair state is final after the search: a fragment it turns from NoMatch into Unique leaves u.tsv"""
    scores = 1
    g, b1, b2, planted = mw.search_workload("families", True, (100, 80), 32, 3)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-insert_min", str(mw.MIN_INS), "-insert_max", str(mw.MAX_INS), "-e", "3", "-s", "2", "-l", "32",
            "-q", str(scores)]
    f = mw.oracle_lists(ora, g, b1, b2, 32, 3, scores, 2)
    fm = ora.filter_mult(2, 3)
    args = (b1, b2, mw.MIN_INS, mw.MAX_INS, scores, fm, 32, 3)
    off, _ = mc.check_pairs_search(ora, {0: g}, [f], *args, search=False)
    on, _ = mc.check_pairs_search(ora, {0: g}, [f], *args)
    s1, s2 = _singles([f], b1, b2, scores, fm)                                   # seed hits only, with and without the search
    got = {}
    for name, flags in (("off", []), ("on", ["-mate_search", "1"])):
        out, plain, u = (str(tmp_path / (name + x)) for x in (".tsv", "_plain.tsv", "_u.tsv"))
        r0 = cli._run(base + ["-o", plain] + flags)
        r = cli._run(base + ["-o", out, "-unpaired", u] + flags)
        assert r0.returncode == 0 and r.returncode == 0, r.stderr.decode()[-2000:]
        assert open(out, "rb").read() == open(plain, "rb").read()
        got[name] = open(u).read().split("\n")[:-1]
    want_off = unpaired_lines(off, s1, s2, [g], b1, b2, scores)
    want_on = unpaired_lines(on, s1, s2, [g], b1, b2, scores)
    assert got["off"] == want_off and got["on"] == want_on
    turned = [i for i in planted["A"] if off["state"][i] == pc.NOMATCH and on["state"][i] == pc.UNIQUE]
    assert len(turned) >= 5, (len(turned), len(planted["A"]))
    ids_off, ids_on = (set(l.split("\t")[0] for l in ls) for ls in (want_off, want_on))
    gone = [i for i in turned if (b1.ids[i] in ids_off or b2.ids[i] in ids_off)]
    assert len(gone) >= 5 and not any(b1.ids[i] in ids_on or b2.ids[i] in ids_on for i in turned)


def test_real_cli_unpaired_loud_errors(tmp_path):
    g = synth.random_genome(60_000, seed=7)
    b1, b2 = synth.sample_pairs(g, 50, 100, 100, 300, 30, 0.0, 8)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    out, u = str(tmp_path / "out.tsv"), str(tmp_path / "u.tsv")
    base = [cli.REAL, "-t", fa, "-o", out, "-Q", "33", "-insert_min", "150", "-insert_max", "420", "-p", p1]
    assert cli._run(base + ["-p2", p2, "-unpaired", u]).returncode == 0
    for args, word in ((["-unpaired", u], b"-p2"), (["-p2", p2, "-unpaired", u, "-pairs_all", "1"], b"-pairs_all"),
                       (["-p2", p2, "-unpaired", out], b"same file as -o")):
        r = cli._run(base + args)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr.decode()[-500:])
