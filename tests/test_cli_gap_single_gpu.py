"""End-to-end: `real -p reads -gapped_single g.tsv`.  g.tsv holds one line per read the anchored gap placement places uniquely,
built here from the checker's records (gap_anchor_checker.py over the oracle's info words and its matchAll lists of the sub-read
batch, index block by index block); -o is byte for byte what it is without the flag."""
import re

import pytest

import gap_anchor_checker as gac
import gap_anchor_workloads as gaw
import gap_checker as gc
import test_cli_pairs_gpu as cli
from real_amd import synth

pytestmark = pytest.mark.gpu

FLAGS = ["-e", str(gaw.TOTALKMAX), "-s", "2", "-l", "32", "-q", "0", "-filter_level", "0", "-Q", "33"]


def single_lines(rec, genomes, b):
    lines = []
    for i in range(b.n_reads):
        r = rec[i]
        if gc.state_of(r["tag"]) != gc.UNIQUE:
            continue
        g = genomes[int(r["fileid"])]
        l = int(b.offsets[i + 1]) - int(b.offsets[i])
        lines.append("\t".join([b.ids[i], "-" if gc.inverted_of(r["tag"]) else "+", g.frag_names[int(r["frag"])],
                                str(int(r["pos"]) - int(g.frag_start[int(r["frag"])]) + 1), gc.cigar_of(r, l), str(int(r["k"]) + abs(int(r["gap"]))),
                                str(int(r["k"])), str(int(r["cost"])), "*" if int(r["second"]) == gc.NONE else str(int(r["second"]))]))
    return lines


def expected(ora, w, ap, genomes, per_block=1 << 62):
    """(lines, summary) of a run over the genome files `genomes`, file ids in their order"""
    info, blocks = gaw.oracle_run(ora, w, ap.anchor_len, [(g, fid) for fid, g in enumerate(genomes)], per_block)
    rec, ctrs = None, []
    for fid, g, hits, hoff in blocks:
        rec, ctr = gac.check_anchor(gc.Text(g.sym, g.frag_start, fid), w["b"], info, hits, hoff, w["prm"], ap, out=rec)
        ctrs.append(ctr)
    st = gc.state_of(rec["tag"])
    summary = "gap single: eligible=%d anchored=%d crowded=%d placed=%d unique=%d gapped=%d\n" % (
        ctrs[0]["eligible"], sum(c["eligible"] - c["skipped"] - c["crowded"] - c["unanchored"] for c in ctrs), sum(c["crowded"] for c in ctrs),
        int((st != gc.NOMATCH).sum()), int((st == gc.UNIQUE).sum()), int(((st != gc.NOMATCH) & (rec["gap"] != 0)).sum()))
    return single_lines(rec, genomes, w["b"]), summary, len(blocks)


def _reads(tmp_path, b):
    p = str(tmp_path / "reads.fq")
    synth.reads_to_fastq(b, p)
    return p


@pytest.mark.parametrize("extra,gap,prm,ap,blocks", [
    ([], [], None, gac.AnchorParams(32, 32), 1),
    (["-batch", "100", "-block", "80000"], ["-gap_max", "16", "-gap_flank", "6", "-gap_margin", "2", "-gap_anchor", "42", "-gap_anchors", "64"],
     gc.Params(16, 6, 4, 6, 1, 4 * gaw.TOTALKMAX + 6 + 16, 2), gac.AnchorParams(42, 64), 2)])
def test_real_cli_gapped_single(ora, tmp_path, extra, gap, prm, ap, blocks):
    w = gaw.workload(seed=5, prm=prm)
    g, b = w["g"], w["b"]
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    base = [cli.REAL, "-t", fa, "-p", _reads(tmp_path, b)] + FLAGS + extra
    plain, out, gfile = str(tmp_path / "plain.tsv"), str(tmp_path / "out.tsv"), str(tmp_path / "g.tsv")
    r = cli._run(base + ["-o", out, "-gapped_single", gfile] + gap)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    if blocks == 1:                                                          # nothing else changes with the flag
        r0 = cli._run(base + ["-o", plain])
        assert r0.returncode == 0 and open(plain, "rb").read() == open(out, "rb").read() and b"gap single" not in r0.stderr
    want, summary, n_blocks = expected(ora, w, ap, [g], 80000 if blocks == 2 else 1 << 62)
    got = open(gfile).read().split("\n")[:-1]
    assert n_blocks == blocks and len(want) >= 60 and got == want
    assert any("D" in l.split("\t")[4] for l in want) and any("I" in l.split("\t")[4] for l in want)
    assert {l.split("\t")[1] for l in want} == {"+", "-"}
    assert summary in r.stderr.decode(), (summary, r.stderr.decode()[-600:])


def test_real_cli_gapped_single_genome_directory(ora, tmp_path):
    """two genome files: every file's blocks fold into one array"""
    wa, wb = gaw.workload(seed=1, n=60), gaw.workload(seed=2, n=60)
    reads = [w["b"].read(i) for w in (wa, wb) for i in range(w["b"].n_reads)]
    both = dict(wa, b=gaw.Batch(reads, ["r%d" % i for i in range(len(reads))]))
    d = tmp_path / "genomes"
    d.mkdir()
    synth.genome_to_fasta(wa["g"], str(d / "a.fa"))
    synth.genome_to_fasta(wb["g"], str(d / "b.fa"))
    out, gfile = str(tmp_path / "out.tsv"), str(tmp_path / "g.tsv")
    r = cli._run([cli.REAL, "-t", str(d), "-p", _reads(tmp_path, both["b"]), "-o", out, "-gapped_single", gfile] + FLAGS)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    order = re.findall(r"Processing file \S*/([ab])\.fa", r.stderr.decode())     # the file ids follow the directory's own order
    assert sorted(set(order)) == ["a", "b"]
    genomes = [{"a": wa["g"], "b": wb["g"]}[x] for x in order[:2]]
    want, summary, _ = expected(ora, both, gac.AnchorParams(32, 32), genomes)
    assert open(gfile).read().split("\n")[:-1] == want and len(want) >= 120
    assert summary in r.stderr.decode(), (summary, r.stderr.decode()[-600:])


def test_real_cli_gapped_single_loud_errors(tmp_path):
    g = synth.random_genome(60_000, seed=7)
    b1, b2 = synth.sample_pairs(g, 50, 100, 100, 300, 30, 0.0, 8)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    out, gfile = str(tmp_path / "out.tsv"), str(tmp_path / "g.tsv")
    base = [cli.REAL, "-t", fa, "-o", out, "-Q", "33", "-p", p1]
    ok = cli._run(base + ["-gapped_single", gfile])
    assert ok.returncode == 0 and b"gap single: eligible=" in ok.stderr, ok.stderr.decode()[-600:]
    for args, word in ((["-p2", p2, "-gapped_single", gfile], b"-gapped"), (["-gapped_single", out], b"same file as -o"),
                       (["-gapped_single", gfile, "-gap_anchor", "0"], b"-gap_anchor"), (["-gapped_single", gfile, "-gap_anchor", "321"], b"-gap_anchor"),
                       (["-gapped_single", gfile, "-gap_anchors", "65"], b"-gap_anchors"), (["-gapped_single", gfile, "-gap_max", "17"], b"-gap_max"),
                       (["-gap_anchor", "40"], b"need -gapped_single"),
                       (["-gapped", gfile], b"-gapped is only meaningful with -p2")):      # (as before this flag existed)
        r = cli._run(base + args)
        assert r.returncode != 0 and word in r.stderr and b"Processing file" not in r.stderr, (args, r.stderr.decode()[-500:])
