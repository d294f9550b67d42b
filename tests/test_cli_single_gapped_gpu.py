"""End-to-end, single-end: `real -p reads -gapped_single g.tsv -sam x.sam -sam_gapped 1 -pileup s.tsv -pileup_depth d.tsv -vcf x.vcf
-pileup_gapped 1 -vcf_indels 1 [-dedup 1]`.  Every file and every summary line is the checkers'
(single_gapped_checker over the oracle's info words and gap_anchor_checker's records, dup_gapped_checker's marks); -o and the
-gapped_single file are byte for byte what they are with -gapped_single alone; without a consumer -dedup 1 marks as it did.
Child processes only."""
import re

import numpy as np
import pytest

import call_checker as ck
import dup_checker as dk
import dup_gapped_checker as dgk
import gap_checker as gc
import indel_checker as ic
import pileup_checker as pk
import pileup_gapped_checker as pgc
import sam_checker as sk
import single_gapped_checker as sgc
import single_gapped_workloads as sw
import test_cli_pairs_gpu as cli
from real_amd import synth

pytestmark = pytest.mark.gpu

MINQ = 20
CONSUMERS = ["-sam_gapped", "1", "-pileup_gapped", "1", "-vcf_indels", "1", "-pileup_minq", str(MINQ)]


def _names(g):
    return [s.split()[0] for s in g.frag_names]


def _contigs(genomes):
    return [(name, int(g.frag_start[k + 1] - g.frag_start[k])) for g in genomes for k, name in enumerate(_names(g))]


def _same(got: str, want: str, what: str):
    """two files line by line (no diff of megabytes on a failure)"""
    a, b = got.split("\n"), want.split("\n")
    first = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), None)
    assert first is None, "%s: line %d: got %r, want %r" % (what, first, a[first], b[first])
    assert len(a) == len(b), "%s: %d lines, want %d" % (what, len(a), len(b))


def _outs(tmp_path, pre):
    f = [str(tmp_path / (pre + n)) for n in ("out.tsv", "g.tsv", "x.sam", "x.vcf", "sites.tsv", "depth.tsv")]
    return f, ["-o", f[0], "-gapped_single", f[1], "-sam", f[2], "-vcf", f[3], "-pileup", f[4], "-pileup_depth", f[5]]


def _inputs(tmp_path, genomes, b):
    """the genome file (or a directory of them, a.fa, b.fa, ...) and the read file"""
    if len(genomes) == 1:
        t = str(tmp_path / "genome.fa")
        synth.genome_to_fasta(genomes[0], t)
    else:
        d = tmp_path / "genomes"
        d.mkdir()
        for k, g in enumerate(genomes):
            synth.genome_to_fasta(g, str(d / ("%s.fa" % "ab"[k])))
        t = str(d)
    p = str(tmp_path / "reads.fq")
    synth.reads_to_fastq(b, p)
    return t, p


def _check_files(files, err, genomes, fnames, b, info, gaps, dup):
    """the -sam, -vcf, -pileup and -pileup_depth files and the summary lines of a run over `genomes` against the checkers; dup: the
    marks of -dedup 1 (None: a run without)"""
    text, ctrs = sgc.sam_single_gapped(genomes, b, info, gaps, dup)
    _same(open(files[2]).read(), text, "-sam")
    assert (sgc.sam_gapped_line(ctrs) + "\n") in err, err[-800:]
    sites, depth, vcf = [], [], [ic.vcf_header(_contigs(genomes))]
    for fid, g in enumerate(genomes):
        pu, cl, ind = sgc.file_expected(g, fid, b, info, gaps, dup, MINQ)
        sites.append(pk.pileup_lines(pu, g.frag_start, g.frag_names))
        depth.append(pk.depth_lines(pu, g.frag_start, g.frag_names))
        vcf.append(ic.vcf_lines_merged(cl.calls(), ind.calls(), g.sym, g.frag_start, _names(g)))
        for line in (pk.stderr_line(pu, fnames[fid]), pgc.stderr_line(pu, fnames[fid]), ck.stderr_line(cl, fnames[fid]), ic.stderr_line(ind, fnames[fid])):
            assert (line + "\n") in err, (line, err[-1500:])
    _same(open(files[4]).read(), "".join(sites), "-pileup")
    _same(open(files[5]).read(), "".join(depth), "-pileup_depth")
    _same(open(files[3]).read(), "".join(vcf), "-vcf")
    return text


_PLAIN = {}


def _plain(tmp_path_factory):
    """-o and the -gapped_single file of the run with -gapped_single alone, once"""
    if not _PLAIN:
        tmp = tmp_path_factory.mktemp("plain")
        w = sw.workload()
        t, p = _inputs(tmp, [w.g], w.b)
        out, gfile = str(tmp / "out.tsv"), str(tmp / "g.tsv")
        r = cli._run([cli.REAL, "-t", t, "-p", p, "-o", out, "-gapped_single", gfile] + sw.FLAGS)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        _PLAIN["x"] = (open(out, "rb").read(), open(gfile, "rb").read(), re.search(r"gap single: .*\n", r.stderr.decode()).group(0))
    return _PLAIN["x"]


@pytest.mark.parametrize("dedup", [1, 0])
def test_real_cli_single_gapped_consumers(ora, tmp_path, tmp_path_factory, dedup):
    w = sw.workload()
    info, gaps, sums, dup, st, _ = sw.expected(ora)
    t, p = _inputs(tmp_path, [w.g], w.b)
    files, args = _outs(tmp_path, "")
    r = cli._run([cli.REAL, "-t", t, "-p", p] + args + sw.FLAGS + CONSUMERS + (["-dedup", "1"] if dedup else []))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    err = r.stderr.decode()
    text = _check_files(files, err, [w.g], [t], w.b, info, gaps, dup if dedup else None)
    # -o and the -gapped_single file do not change, nor does the pass's summary line
    out0, g0, line0 = _plain(tmp_path_factory)
    assert open(files[0], "rb").read() == out0 and open(files[1], "rb").read() == g0 and len(g0) > 10_000 and line0 in err
    assert err.index("All done.") < err.index("pileup:") < err.index("sam:") < err.index("gap single:")
    if dedup:
        assert (dk.stderr_line(st, sw.MIN_QUAL) + "\n" + dgk.gapped_line(info, gaps, sums, dup) + "\n") in err, err[-1500:]
        assert err.index("duplicates:") < err.index("pileup:")
        flags = [int(l.split("\t")[1]) for l in text.split("\n") if l and not l.startswith("@")]
        assert sum(1 for f in flags if f & 1024) == st["duplicates"] and 4 + 1024 not in flags
    else:
        assert "duplicates" not in err
    assert not any(l.split("\t")[1] == "4" and l.split("\t")[0] in {w.b.ids[i] for i in np.nonzero(gc.state_of(gaps["tag"]) == gc.UNIQUE)[0]}
                   for l in text.split("\n") if l and not l.startswith("@"))


def test_real_cli_dedup_without_a_consumer_marks_as_before(ora, tmp_path):
    """-dedup 1 -gapped_single and none of the three flags: the marks of real_hip_mark_duplicates, the gapped reads FLAG 4"""
    w = sw.workload()
    info, gaps, sums, _, _, _ = sw.expected(ora)
    t, p = _inputs(tmp_path, [w.g], w.b)
    out, gfile, sam = (str(tmp_path / n) for n in ("out.tsv", "g.tsv", "x.sam"))
    r = cli._run([cli.REAL, "-t", t, "-p", p, "-o", out, "-gapped_single", gfile, "-sam", sam, "-dedup", "1"] + sw.FLAGS)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    dup, st, _ = dk.mark_single(info, sums)
    plain, _ = sk.sam_single([w.g], w.b, info, None, False)
    _same(open(sam).read(), dk.sam_with_marks(plain, {w.b.ids[i] for i in np.nonzero(dup)[0]}), "-sam")
    err = r.stderr.decode()
    assert (dk.stderr_line(st, sw.MIN_QUAL) + "\n") in err and "duplicates gapped" not in err and "sam gapped" not in err
    assert err.index("sam:") < err.index("Obtained", err.index("sam:")) < err.index("gap single:")      # the gapped pass runs where it ran


def test_real_cli_single_gapped_two_genome_files(ora, tmp_path):
    """records of both files: each read's line in its record's pass, none twice; every file's pass sees all records"""
    w = sw.two_files()
    t, p = _inputs(tmp_path, [w.g, w.g2], w.b)
    files, args = _outs(tmp_path, "")
    r = cli._run([cli.REAL, "-t", t, "-p", p] + args + sw.FLAGS + CONSUMERS + ["-dedup", "1"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    err = r.stderr.decode()
    order = re.findall(r"Processing file (\S*/([ab])\.fa)", err)            # the file ids follow the directory's own order
    assert sorted({x for _, x in order}) == ["a", "b"]
    genomes = [{"a": w.g, "b": w.g2}[x] for _, x in order[:2]]
    fnames = [f for f, _ in order[:2]]
    info, gaps, _ = sw.oracle_run(ora, w.b, genomes, w.prm)
    unique = gc.state_of(gaps["tag"]) == gc.UNIQUE
    assert all(int((unique & (gaps["fileid"] == f) & (gaps["gap"] != 0)).sum()) >= 50 for f in (0, 1))
    sums = dk.summaries_of(w.b, sw.MIN_QUAL)
    dup, st, _ = dgk.mark_groups(info, gaps, sums)
    assert int(dup[unique].sum()) >= 5
    text = _check_files(files, err, genomes, fnames, w.b, info, gaps, dup)
    names = [l.split("\t")[0] for l in text.split("\n") if l and not l.startswith("@")]
    assert sorted(names) == sorted(w.b.ids)                                  # one line per read
    assert (dk.stderr_line(st, sw.MIN_QUAL) + "\n" + dgk.gapped_line(info, gaps, sums, dup) + "\n") in err


def test_real_cli_single_gapped_two_index_blocks(ora, tmp_path):
    w = sw.workload()
    info, gaps, sums, dup, st, _ = sw.expected(ora)
    i2, g2, blocks = sw.oracle_run(ora, w.b, [w.g], w.prm, per_block=20_000)
    assert blocks == 2 and np.array_equal(i2, info) and g2.tobytes() == gaps.tobytes()
    t, p = _inputs(tmp_path, [w.g], w.b)
    files, args = _outs(tmp_path, "")
    r = cli._run([cli.REAL, "-t", t, "-p", p] + args + sw.FLAGS + CONSUMERS + ["-dedup", "1", "-block", "20000", "-batch", "3000"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    err = r.stderr.decode()
    assert err.count("Obtained") == 4                                        # two blocks in the matching pass, two in the gapped one
    _check_files(files, err, [w.g], [t], w.b, info, gaps, dup)
    assert (dgk.gapped_line(info, gaps, sums, dup) + "\n") in err


def test_real_cli_single_gapped_loud_refusals(tmp_path):
    g = synth.random_genome(60_000, seed=7)
    b1, b2 = synth.sample_pairs(g, 50, 100, 100, 300, 30, 0.0, 8)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    out, gfile, sam, vcf, sites = (str(tmp_path / n) for n in ("out.tsv", "g.tsv", "x.sam", "x.vcf", "s.tsv"))
    base = [cli.REAL, "-t", fa, "-o", out, "-Q", "33", "-p", p1]
    for args, word in ((["-sam", sam, "-sam_gapped", "1"], b"needs -gapped_single"), (["-vcf", vcf, "-vcf_indels", "1"], b"needs -gapped_single"),
                       (["-pileup", sites, "-pileup_gapped", "1"], b"needs -gapped_single"),
                       (["-pileup", sites, "-pileup_gapped", "1"], b"single-end drivers are not there yet"),
                       (["-gapped_single", gfile, "-sam_gapped", "1"], b"needs -sam"), (["-gapped_single", gfile, "-vcf_indels", "1"], b"needs -vcf"),
                       (["-gapped_single", gfile, "-pileup_gapped", "1"], b"needs one of -pileup / -pileup_depth / -vcf"),
                       (["-p2", p2, "-gapped_single", gfile, "-vcf", vcf, "-vcf_indels", "1"], b"-gapped_single places single reads")):
        r = cli._run(base + args)
        assert r.returncode != 0 and word in r.stderr and b"Processing file" not in r.stderr, (args, r.stderr.decode()[-500:])
