"""End-to-end: `real -p mates1 -p2 mates2 -sam x.sam -gapped g.tsv -sam_gapped 1`.  The whole SAM file is the checker's
(gapped_list_checker.sam_pairs_gapped over the gap checker's records of the oracle's lists), line for line; every rescued line
rebuilds the genome text from SEQ, CIGAR and MD alone; -o, -unpaired, the -gapped file and its summary are what they are without
the flag, and so is the -sam file of a run with -gapped but without -sam_gapped."""
import re

import pytest

import gap_checker as gc
import gap_workloads as gw
import gapped_list_checker as glc
import gapped_list_workloads as glw
import sam_checker as sk
import test_cli_gap_gpu as gap_cli
import test_cli_pairs_gpu as cli
from real_amd import synth

pytestmark = pytest.mark.gpu

FLAGS = gap_cli.FLAGS


def _same_text(got, want):
    g, w = got.split("\n"), want.split("\n")
    for k, (a, b) in enumerate(zip(g, w)):
        assert a == b, (k, a, b)
    assert len(g) == len(w)


def _check_rescued_lines(text, genomes, min_ins, max_ins):
    """what holds for every rescued mate and its anchor, from the file alone -> the rescued lines"""
    letters = {}                                                          # (two genome files may name their fragments alike: a list per name)
    for g in genomes:
        for f, name in enumerate(g.frag_names):
            letters.setdefault(sk.frag_name(name), []).append("".join("ACGTN"[c] for c in g.sym[int(g.frag_start[f]):int(g.frag_start[f + 1])]))
    by_name, rescued = {}, []
    for l in text.split("\n")[:-1]:
        if l.startswith("@"):
            continue
        f = l.split("\t")
        by_name.setdefault(f[0], []).append(f)
        if any(x.startswith("ZC:i:") for x in f[11:]):
            rescued.append(f)
    for f in rescued:
        md = [x for x in f if x.startswith("MD:Z:")][0][5:]
        nm = int([x for x in f if x.startswith("NM:i:")][0][5:])
        assert glc.MD_RE.match(md) and not any(x.startswith("ZS:f:") for x in f)
        ref = glc.reference_from_cigar_md(f[9], f[5], md)
        pos = int(f[3]) - 1
        assert any(ref == t[pos:pos + len(ref)] for t in letters[f[2]]), f[0]
        ops = re.findall(r"(\d+)([MID])", f[5])
        assert nm == sum(c.isalpha() for c in md.replace("^", "")) + sum(int(a) for a, b in ops if b == "I")
        assert f[4] == "255"
        mates = by_name[f[0]]
        assert len(mates) == 2
        a = mates[0] if mates[1] is f else mates[1]
        fl, afl = int(f[1]), int(a[1])
        assert int(f[8]) + int(a[8]) == 0 and int(f[8]) != 0                                 # TLEN of the two mates sums to 0
        assert not (fl & 4) and not (fl & 8) and not (afl & 4) and not (afl & 8)
        assert bool(fl & 16) == bool(afl & 32) and bool(afl & 16) == bool(fl & 32) and bool(fl & 16) != bool(afl & 16)
        outer = int(a[8]) if fl & 16 else int(f[8])                                          # the forward mate's TLEN
        assert (fl & 2) == (afl & 2) and bool(fl & 2) == (min_ins <= outer <= max_ins)
        assert (fl & 192) | (afl & 192) == 192 and fl & 1 and afl & 1
        assert (f[6], f[7]) == ("=", a[3]) and (a[6], a[7]) == ("=", f[3]) and a[2] == f[2]
    return rescued


_ONE = {}


def _one_file(ora):
    """the one-file workload, its records and both SAM files of the checker: computed once for the parametrised cases"""
    if not _ONE:
        w = glw.workload(seed=5)
        g, b1, b2 = w["g"], w["b1"], w["b2"]
        pairs, s1, s2, _ = gw.oracle_records(ora, w)
        rec, ctr = gc.check_gap(gc.Text(g.sym, g.frag_start, 0), b1, b2, pairs, s1, s2, w["min_ins"], w["max_ins"], w["prm"])
        plain_sam, _ = sk.sam_pairs([g], b1, b2, pairs, s1, s2, False)
        want, ctrs = glc.sam_pairs_gapped([g], b1, b2, pairs, s1, s2, rec, w["min_ins"], w["max_ins"], False)
        _ONE["x"] = (w, ctr, plain_sam, want, ctrs)
    return _ONE["x"]


@pytest.mark.parametrize("extra", [[], ["-batch", "100"]])
def test_real_cli_sam_gapped(ora, tmp_path, extra):
    w, ctr, plain_sam, want, ctrs = _one_file(ora)
    g, b1, b2 = w["g"], w["b1"], w["b2"]
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-insert_min", str(w["min_ins"]), "-insert_max", str(w["max_ins"])] + FLAGS + extra
    names = ("out.tsv", "u.tsv", "g.tsv")
    plain = [str(tmp_path / ("plain_" + n)) for n in names]
    flagged = [str(tmp_path / n) for n in names]
    sam1, sam2 = (str(tmp_path / n) for n in ("plain.sam", "x.sam"))
    r1 = cli._run(base + ["-o", plain[0], "-unpaired", plain[1], "-sam", sam1, "-gapped", plain[2]])
    r = cli._run(base + ["-o", flagged[0], "-unpaired", flagged[1], "-sam", sam2, "-gapped", flagged[2], "-sam_gapped", "1"])
    assert r1.returncode == 0 and r.returncode == 0, r.stderr.decode()[-2000:]
    for a, b in zip(plain, flagged):
        assert open(a, "rb").read() == open(b, "rb").read(), b                 # -o, -unpaired and the -gapped file do not change with the flag
    _same_text(open(sam1).read(), plain_sam)                                   # -sam with -gapped but without -sam_gapped is today's: sam_checker's file
    got = open(sam2).read()
    _same_text(got, want)
    rescued = _check_rescued_lines(got, [g], w["min_ins"], w["max_ins"])
    assert len(rescued) >= 60 and len(rescued) == ctr["unique"]
    assert any("D" in f[5] for f in rescued) and any("I" in f[5] for f in rescued)
    assert any(re.search(r"\^[A-Z]+0[A-Z]", [x for x in f if x.startswith("MD:Z:")][0]) for f in rescued)
    err = r.stderr.decode()
    assert gap_cli._summary([ctr]) in err and gap_cli._summary([ctr]) in r1.stderr.decode()      # the rescue ran once: the counters are not doubled
    assert glc.stderr_line(ctrs) + "\n" in err and ctrs[0]["disagree"] == 0 and ctrs[0]["placed"] == len(rescued)
    assert b"sam gapped" not in r1.stderr


def test_real_cli_sam_gapped_genome_directory(ora, tmp_path):
    """two genome files: the pass of a file rescues, lists and writes the fragments whose anchor lies in it"""
    wa, wb = glw.workload(seed=1, n=100), glw.workload(seed=2, n=100)
    reads = [[w[k].read(i) for w in (wa, wb) for i in range(w[k].n_reads)] for k in ("b1", "b2")]
    ids = ["f%d" % i for i in range(len(reads[0]))]
    b1, b2 = gw.Batch(reads[0], [x + "/1" for x in ids]), gw.Batch(reads[1], [x + "/2" for x in ids])
    d = tmp_path / "genomes"
    d.mkdir()
    synth.genome_to_fasta(wa["g"], str(d / "a.fa"))
    synth.genome_to_fasta(wb["g"], str(d / "b.fa"))
    p1, p2 = cli._write(tmp_path, b1, b2)
    base = [cli.REAL, "-t", str(d), "-p", p1, "-p2", p2, "-insert_min", str(gw.MIN_INS), "-insert_max", str(gw.MAX_INS)] + FLAGS
    out0, g0, out, gfile, sam = (str(tmp_path / n) for n in ("out0.tsv", "g0.tsv", "out.tsv", "g.tsv", "x.sam"))
    r0 = cli._run(base + ["-o", out0, "-gapped", g0])
    r = cli._run(base + ["-o", out, "-gapped", gfile, "-sam", sam, "-sam_gapped", "1"])
    assert r0.returncode == 0 and r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out0, "rb").read() == open(out, "rb").read() and open(g0, "rb").read() == open(gfile, "rb").read()
    order = re.findall(r"Processing file \S*/([ab])\.fa", r.stderr.decode())     # the file ids follow the directory's own order
    genomes = [{"a": wa["g"], "b": wb["g"]}[x] for x in order[:2]]
    assert sorted(order[:2]) == ["a", "b"]
    both = dict(wa, b1=b1, b2=b2)
    files, rec, gctrs = None, None, []
    for fid, g in enumerate(genomes):
        pairs, s1, s2, files = gw.oracle_records(ora, both, g=g, fileid=fid, prev=files)
    for fid, g in enumerate(genomes):
        rec, c = gc.check_gap(gc.Text(g.sym, g.frag_start, fid), b1, b2, pairs, s1, s2, gw.MIN_INS, gw.MAX_INS, both["prm"], out=rec)
        gctrs.append(c)
    want, ctrs = glc.sam_pairs_gapped(genomes, b1, b2, pairs, s1, s2, rec, gw.MIN_INS, gw.MAX_INS, False)
    got = open(sam).read()
    _same_text(got, want)
    rescued = _check_rescued_lines(got, genomes, gw.MIN_INS, gw.MAX_INS)
    assert all(c["placed"] >= 20 for c in ctrs) and ctrs[1]["other_file"] >= 20 and len(rescued) == sum(c["placed"] for c in ctrs)
    err = r.stderr.decode()
    assert gap_cli._summary(gctrs) in err and gap_cli._summary(gctrs) in r0.stderr.decode() and glc.stderr_line(ctrs) + "\n" in err


def test_real_cli_sam_gapped_loud_errors(tmp_path):
    g = synth.random_genome(60_000, seed=7)
    b1, b2 = synth.sample_pairs(g, 50, 100, 100, 300, 30, 0.0, 8)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    out, gfile, sam = (str(tmp_path / n) for n in ("out.tsv", "g.tsv", "x.sam"))
    base = [cli.REAL, "-t", fa, "-o", out, "-Q", "33", "-insert_min", "150", "-insert_max", "420", "-p", p1]
    ok = cli._run(base + ["-p2", p2, "-gapped", gfile, "-sam", sam, "-sam_gapped", "1"])
    assert ok.returncode == 0 and b"sam gapped: mates=" in ok.stderr and b"gap rescue: eligible=" in ok.stderr
    for args, word in ((["-sam", sam, "-gapped", gfile, "-sam_gapped", "1"], b"-p2"), (["-p2", p2, "-gapped", gfile, "-sam_gapped", "1"], b"needs -sam"),
                       (["-p2", p2, "-sam", sam, "-sam_gapped", "1"], b"needs -gapped"),
                       (["-p2", p2, "-sam", sam, "-gapped", gfile, "-sam_gapped", "1", "-pairs_all", "1"], b"-pairs_all")):
        r = cli._run(base + args)
        assert r.returncode != 0 and word in r.stderr and b"Processing file" not in r.stderr, (args, r.stderr.decode()[-500:])
