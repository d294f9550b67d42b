"""End-to-end: `real -p mates1 -p2 mates2 -vcf x.vcf -vcf_indels 1 [-vcf_minalt N]`.  The whole VCF file is the checker's
(indel_checker over the gap checker's records of the oracle's lists, merged with call_checker's SNP lines), for one genome file and
for a directory of two; every indel line is rebuilt against the genome; -o, -sam, -gapped and the SNP lines are what they are
without the flag; with -sam_gapped 1 and -gapped beside it the rescue still runs once.  Child processes only."""
import re

import numpy as np
import pytest

import call_checker as ck
import gap_checker as gc
import indel_checker as ic
import indel_workloads as iw
import pileup_checker as pk
import test_cli_gap_gpu as gap_cli
import test_cli_pairs_gpu as cli
from real_amd import synth

pytestmark = pytest.mark.gpu

MATCH = ["-e", str(iw.TOTALKMAX), "-s", str(iw.SEEDKMAX), "-l", str(iw.SEEDL), "-q", "0", "-filter_level", "0", "-Q", "33", "-pileup_minq", "20"]


def _names(g):
    return [s.split()[0] for s in g.frag_names]


def _contigs(genomes):
    return [(name, int(g.frag_start[k + 1] - g.frag_start[k])) for g in genomes for k, name in enumerate(_names(g))]


def _file_expected(g, fid, b1, b2, pairs, rec):
    """(SNP calls checker, indel checker) of one genome file from the final records"""
    pu = pk.Pileup(g.sym, fid, 20)
    pu.add_pairs(b1, b2, pairs)
    cl = ck.Calls(pu)
    cl.add_pairs(b1, b2, pairs)
    ind = ic.Indels(pu, g.frag_start)
    ind.add(b1, b2, rec)
    return cl, ind


_ONE = {}


def _one_file(ora):
    if not _ONE:
        w = iw.planted()
        pairs, s1, s2, _ = iw.oracle_records(ora, w)
        rec, ctr = gc.check_gap(gc.Text(w.g.sym, w.g.frag_start, 0), w.b1, w.b2, pairs, s1, s2, w.min_ins, w.max_ins, w.prm)
        _ONE["x"] = (w, ctr) + _file_expected(w.g, 0, w.b1, w.b2, pairs, rec)
    return _ONE["x"]


def _rebuild(lines, g, plants, w):
    """every indel line against the genome: REF is the text at POS; and ALT put in place of REF gives the planted haplotype"""
    names = _names(g)
    text = ["".join("ACGTN"[c] for c in g.sym[int(g.frag_start[f]):int(g.frag_start[f + 1])]) for f in range(len(names))]
    seen = {}
    for l in lines:
        f = l.split("\t")
        if "INDEL" not in f[7]:
            continue
        t, pos = text[names.index(f[0])], int(f[1]) - 1
        assert t[pos:pos + len(f[3])] == f[3] and f[3][0] == f[4][0] and (len(f[3]) == 1) != (len(f[4]) == 1), l
        dp, sf, sr = (int(x) for x in re.match(r"DP=(\d+);INDEL;SF=(\d+);SR=(\d+)$", f[7]).groups())
        gt, gq, dp2, ad = f[9].split(":")
        assert f[8] == "GT:GQ:DP:AD" and gt in ("0/1", "1/1") and int(dp2) == dp == sum(int(x) for x in ad.split(",")) and sf + sr == int(ad.split(",")[1])
        seen[(f[0], pos)] = (t[:pos] + f[4] + t[pos + len(f[3]):], gt)
    right = 0
    for p in plants:
        f = int(np.searchsorted(np.asarray(g.frag_start, dtype=np.int64), p["x"], side="right")) - 1
        x = p["x"] - int(g.frag_start[f])
        hap = text[f][:x] + "".join("ACGT"[b] for b in p["s"]) + text[f][x + max(p["g"], 0):]
        a, _, _ = iw.planted_key(w, p)
        got = seen.get((names[f], a - int(g.frag_start[f])))
        right += got is not None and got[0] == hap and got[1] == ("1/1" if p["hom"] else "0/1")
    return right


def _inputs(ora, tmp_path):
    w, ctr, cl, ind = _one_file(ora)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(w.g, fa)
    p1, p2 = cli._write(tmp_path, w.b1, w.b2)
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-insert_min", str(w.min_ins), "-insert_max", str(w.max_ins)] + MATCH
    return w, ctr, cl, ind, fa, base


def _outs(tmp_path, pre):
    f = [str(tmp_path / (pre + n)) for n in ("out.tsv", "x.sam", "g.tsv", "x.vcf")]
    return f, ["-o", f[0], "-sam", f[1], "-gapped", f[2], "-vcf", f[3]]


def _whole_vcf(cl, ind, g, *thr):
    snp = cl.calls(*(thr[0], thr[2])) if thr else cl.calls()
    return ic.vcf_header(_contigs([g])) + ic.vcf_lines_merged(snp, ind.calls(*thr), g.sym, g.frag_start, _names(g))


def test_real_cli_vcf_indels(ora, tmp_path):
    w, ctr, cl, ind, fa, base = _inputs(ora, tmp_path)
    g = w.g
    (plain, plain_args), (flagged, flagged_args) = _outs(tmp_path, "plain_"), _outs(tmp_path, "")
    r0 = cli._run(base + plain_args)
    assert r0.returncode == 0, r0.stderr.decode()[-2000:]
    r = cli._run(base + flagged_args + ["-vcf_indels", "1"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    for a, b in zip(plain[:3], flagged[:3]):
        assert open(a, "rb").read() == open(b, "rb").read() and len(open(a, "rb").read()) > 1000, b       # -o, -sam and -gapped do not change
    calls = ind.calls()
    assert cl.calls().shape[0] >= 10, "SNP lines to merge the indel lines with"
    assert open(plain[3]).read() == ck.vcf_header(_contigs([g])) + ck.vcf_lines(cl.calls(), g.frag_start, _names(g))
    got = open(flagged[3]).read()
    assert got == _whole_vcf(cl, ind, g)
    lines = [l for l in got.splitlines() if not l.startswith("#")]
    assert [l for l in lines if "INDEL" not in l.split("\t")[7]] == [l for l in open(plain[3]).read().splitlines() if not l.startswith("#")]
    right = _rebuild(lines, g, w.plants, w)
    print("planted indels written with the planted genotype: %d of %d" % (right, len(w.plants)))
    assert right >= 20 and calls.shape[0] >= 20 and (calls["gap"] > 0).sum() >= 8 and (calls["gap"] < 0).sum() >= 8
    err, err0 = r.stderr.decode(), r0.stderr.decode()
    assert (ic.stderr_line(ind, fa) + "\n") in err and "indels:" not in err0 and (ck.stderr_line(cl, fa) + "\n") in err
    assert err.count("gap rescue:") == 1 and gap_cli._summary([ctr]) in err and gap_cli._summary([ctr]) in err0      # the rescue ran once


def test_real_cli_vcf_indels_beside_sam_gapped(ora, tmp_path):
    """-sam_gapped 1 and -gapped beside the flag: the -sam pass and gapPass find the records made; nothing is doubled, nothing changes"""
    w, ctr, cl, ind, fa, base = _inputs(ora, tmp_path)
    (plain, plain_args), (both, both_args) = _outs(tmp_path, "plain_"), _outs(tmp_path, "both_")
    r1 = cli._run(base + plain_args + ["-sam_gapped", "1"])
    assert r1.returncode == 0, r1.stderr.decode()[-2000:]
    r2 = cli._run(base + both_args + ["-sam_gapped", "1", "-vcf_indels", "1"])
    assert r2.returncode == 0, r2.stderr.decode()[-2000:]
    for a, b in zip(plain[:3], both[:3]):
        assert open(a, "rb").read() == open(b, "rb").read() and len(open(a, "rb").read()) > 1000, b
    assert open(both[3]).read() == _whole_vcf(cl, ind, w.g) and "\tZC:i:" in open(both[1]).read()
    e1, e2 = r1.stderr.decode(), r2.stderr.decode()
    assert e2.count("gap rescue:") == 1 and gap_cli._summary([ctr]) in e2 and gap_cli._summary([ctr]) in e1
    same = re.search(r"sam gapped: .*\n", e1).group(0)
    assert same in e2 and (ic.stderr_line(ind, fa) + "\n") in e2


def test_real_cli_vcf_indels_thresholds(ora, tmp_path):
    """-vcf_minalt, and -vcf_minqual / -vcf_mindepth for both kinds of call; the reads in several batches; no -gapped beside it"""
    w, ctr, cl, ind, fa, base = _inputs(ora, tmp_path)
    vf = str(tmp_path / "t.vcf")
    r = cli._run(base + ["-o", str(tmp_path / "out.tsv"), "-vcf", vf, "-vcf_indels", "1", "-vcf_minalt", "12", "-vcf_minqual", "300", "-vcf_mindepth", "5",
                         "-batch", "500"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert 0 < ind.calls(300, 12, 5).shape[0] < ind.calls().shape[0]
    assert open(vf).read() == _whole_vcf(cl, ind, w.g, 300, 12, 5)
    assert (ic.stderr_line(ind, fa, 300, 12, 5) + "\n") in r.stderr.decode() and b"gap rescue:" not in r.stderr


def test_real_cli_vcf_indels_genome_directory(ora, tmp_path):
    """two genome files: one header, per file its SNP and indel calls merged, the rescue of a file in that file's pass"""
    wa, wb = iw.planted(), iw.planted(8)
    reads = [[getattr(w, k).read(i) for w in (wa, wb) for i in range(getattr(w, k).n_reads)] for k in ("b1", "b2")]
    quals = [[getattr(w, k)._quals[i] for w in (wa, wb) for i in range(getattr(w, k).n_reads)] for k in ("b1", "b2")]
    ids = ["f%d" % i for i in range(len(reads[0]))]
    b1, b2 = iw.Batch(reads[0], quals[0], [x + "/1" for x in ids]), iw.Batch(reads[1], quals[1], [x + "/2" for x in ids])
    d = tmp_path / "genomes"
    d.mkdir()
    synth.genome_to_fasta(wa.g, str(d / "a.fa"))
    synth.genome_to_fasta(wb.g, str(d / "b.fa"))
    p1, p2 = cli._write(tmp_path, b1, b2)
    base = [cli.REAL, "-t", str(d), "-p", p1, "-p2", p2, "-insert_min", str(wa.min_ins), "-insert_max", str(wa.max_ins)] + MATCH
    out0, v0, out, vf = (str(tmp_path / n) for n in ("out0.tsv", "v0.vcf", "out.tsv", "x.vcf"))
    r0 = cli._run(base + ["-o", out0, "-vcf", v0])
    r = cli._run(base + ["-o", out, "-vcf", vf, "-vcf_indels", "1"])
    assert r0.returncode == 0 and r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out0, "rb").read() == open(out, "rb").read()
    order = re.findall(r"Processing file \S*/([ab])\.fa", r.stderr.decode())     # the file ids follow the directory's own order
    genomes = [{"a": wa.g, "b": wb.g}[x] for x in order[:2]]
    assert sorted(order[:2]) == ["a", "b"]
    files, rec = None, None
    for fid, g in enumerate(genomes):
        pairs, s1, s2, files = iw.oracle_records(ora, wa, g=g, fileid=fid, prev=files, b1=b1, b2=b2)
    for fid, g in enumerate(genomes):
        rec, _ = gc.check_gap(gc.Text(g.sym, g.frag_start, fid), b1, b2, pairs, s1, s2, wa.min_ins, wa.max_ins, wa.prm, out=rec)
    want, plain, err = ic.vcf_header(_contigs(genomes)), ck.vcf_header(_contigs(genomes)), r.stderr.decode()
    for fid, g in enumerate(genomes):
        cl, ind = _file_expected(g, fid, b1, b2, pairs, rec)
        assert ind.calls().shape[0] >= 15
        want += ic.vcf_lines_merged(cl.calls(), ind.calls(), g.sym, g.frag_start, _names(g))
        plain += ck.vcf_lines(cl.calls(), g.frag_start, _names(g))
        name = str(d / ("%s.fa" % order[fid]))
        assert any(l.startswith("indels: file=") and l.endswith(ic.stderr_line(ind, "X").split("file=X")[1]) and name in l for l in err.splitlines()), err[-1500:]
    assert open(vf).read() == want and open(v0).read() == plain


def test_real_cli_vcf_indels_loud_refusals(tmp_path):
    g = synth.random_genome(60_000, seed=7)
    b1, b2 = synth.sample_pairs(g, 50, 100, 100, 300, 30, 0.0, 8)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    out, vf = str(tmp_path / "out.tsv"), str(tmp_path / "x.vcf")
    base = [cli.REAL, "-t", fa, "-o", out, "-Q", "33", "-insert_min", "150", "-insert_max", "420", "-p", p1]
    ok = cli._run(base + ["-p2", p2, "-vcf", vf, "-vcf_indels", "1"])
    assert ok.returncode == 0 and b"indels: file=" in ok.stderr and b"calls=0" in ok.stderr and "##INFO=<ID=INDEL" in open(vf).read()
    for args, word in ((["-vcf", vf, "-vcf_indels", "1"], b"-p2"), (["-p2", p2, "-vcf_indels", "1"], b"needs -vcf"),
                       (["-p2", p2, "-vcf", vf, "-vcf_minalt", "3"], b"-vcf_indels 1")):
        r = cli._run(base + args)
        assert r.returncode != 0 and word in r.stderr and b"Processing file" not in r.stderr, (args, r.stderr.decode()[-500:])
