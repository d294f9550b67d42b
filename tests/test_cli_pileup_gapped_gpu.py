"""End-to-end: `real -p mates1 -p2 mates2 -pileup s.tsv -pileup_depth d.tsv -vcf x.vcf -pileup_gapped 1`.  The site file, the depth
file, the VCF file and the summary line are the checker's (pileup_gapped_checker over the gap checker's records of the oracle's
lists); -o, -sam, -gapped and the indel lines of -vcf_indels 1 are byte for byte what they are without the flag; the flag's loud
refusals.  Child processes only."""
import pytest

import call_checker as ck
import gap_checker as gc
import indel_checker as ic
import indel_workloads as iw
import pileup_checker as pk
import pileup_gapped_checker as pgc
import test_cli_gap_gpu as gap_cli
import test_cli_pairs_gpu as cli
import test_cli_vcf_indels_gpu as vcf_cli
from real_amd import synth

pytestmark = pytest.mark.gpu

_ONE = {}


def _expected(ora):
    """the planted workload: the gap checker's records, then the checker's pileup, calls and indel calls with the gapped placements"""
    if not _ONE:
        w = iw.planted()
        pairs, s1, s2, _ = iw.oracle_records(ora, w)
        rec, ctr = gc.check_gap(gc.Text(w.g.sym, w.g.frag_start, 0), w.b1, w.b2, pairs, s1, s2, w.min_ins, w.max_ins, w.prm)
        pu = pgc.GappedPileup(w.g.sym, 0, 20)
        pu.add_pairs(w.b1, w.b2, pairs)
        pu.add_gapped(w.b1, w.b2, rec)
        cl = pgc.GappedCalls(pu)
        cl.add_pairs(w.b1, w.b2, pairs)
        cl.add_gapped(w.b1, w.b2, rec)
        ind = ic.Indels(pu.ungapped_view(), w.g.frag_start)
        ind.add(w.b1, w.b2, rec)
        _ONE["x"] = (w, ctr, pu, cl, ind)
    return _ONE["x"]


def _outs(tmp_path, pre):
    f = [str(tmp_path / (pre + n)) for n in ("out.tsv", "x.sam", "g.tsv", "x.vcf", "sites.tsv", "depth.tsv")]
    return f, ["-o", f[0], "-sam", f[1], "-gapped", f[2], "-vcf", f[3], "-pileup", f[4], "-pileup_depth", f[5]]


def _same(got: str, want: str, what: str):
    """two files line by line (no diff of megabytes on a failure)"""
    a, b = got.split("\n"), want.split("\n")
    first = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), None)
    assert first is None, "%s: line %d: got %r, want %r" % (what, first, a[first], b[first])
    assert len(a) == len(b), "%s: %d lines, want %d" % (what, len(a), len(b))


def test_real_cli_pileup_gapped(ora, tmp_path):
    w, ctr, pu, cl, ind = _expected(ora)
    g, names = w.g, vcf_cli._names(w.g)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, w.b1, w.b2)
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-insert_min", str(w.min_ins), "-insert_max", str(w.max_ins)] + vcf_cli.MATCH + ["-vcf_indels", "1"]
    (plain, plain_args), (flagged, flagged_args) = _outs(tmp_path, "plain_"), _outs(tmp_path, "")
    r0 = cli._run(base + plain_args)
    assert r0.returncode == 0, r0.stderr.decode()[-2000:]
    r = cli._run(base + flagged_args + ["-pileup_gapped", "1", "-batch", "700"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    for a, b in zip(plain[:3], flagged[:3]):
        assert open(a, "rb").read() == open(b, "rb").read() and len(open(a, "rb").read()) > 1000, b       # -o, -sam and -gapped do not change
    # the site file, the depth file and the VCF file are the checker's
    _same(open(flagged[4]).read(), pk.pileup_lines(pu, g.frag_start, g.frag_names), "-pileup")
    _same(open(flagged[5]).read(), pk.depth_lines(pu, g.frag_start, g.frag_names), "-pileup_depth")
    want_vcf = ic.vcf_header(vcf_cli._contigs([g])) + ic.vcf_lines_merged(cl.calls(), ind.calls(), g.sym, g.frag_start, names)
    got_vcf = open(flagged[3]).read()
    _same(got_vcf, want_vcf, "-vcf")
    # ... and they differ from the files without the flag, but for the indel lines
    assert (open(plain[4]).read() != open(flagged[4]).read()) and (open(plain[5]).read() != open(flagged[5]).read())

    def indel_lines(text):
        return [l for l in text.splitlines() if not l.startswith("#") and "INDEL" in l.split("\t")[7]]
    assert indel_lines(got_vcf) == indel_lines(open(plain[3]).read()) and len(indel_lines(got_vcf)) >= 20
    err, err0 = r.stderr.decode(), r0.stderr.decode()
    assert (pgc.stderr_line(pu, fa) + "\n") in err and "pileup gapped:" not in err0
    assert (pk.stderr_line(pu, fa) + "\n") in err and (ic.stderr_line(ind, fa) + "\n") in err and (ic.stderr_line(ind, fa) + "\n") in err0
    assert (ck.stderr_line(cl, fa) + "\n") in err
    assert err.count("gap rescue:") == 1 and gap_cli._summary([ctr]) in err and gap_cli._summary([ctr]) in err0      # the rescue ran once
    assert pu.gstats["placed"] > 200 and pu.gstats["deleted"] > 100 and pu.gstats["inserted"] > 100


def test_real_cli_pileup_gapped_without_the_other_passes(ora, tmp_path):
    """no -vcf_indels, no -gapped, no -sam beside it: the pileup pass runs the rescue itself; -pileup_depth alone is enough (the depth
    knows no quality filter: -pileup_minq, which needs -pileup or -vcf, is left out of that run)"""
    w, ctr, pu, cl, ind = _expected(ora)
    g, names = w.g, vcf_cli._names(w.g)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, w.b1, w.b2)
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-insert_min", str(w.min_ins), "-insert_max", str(w.max_ins)] + vcf_cli.MATCH
    out, depth, vf = (str(tmp_path / n) for n in ("out.tsv", "depth.tsv", "x.vcf"))
    r = cli._run(base[:-2] + ["-o", out, "-pileup_depth", depth, "-pileup_gapped", "1"])
    assert r.returncode == 0 and vcf_cli.MATCH[-2] == "-pileup_minq", r.stderr.decode()[-2000:]
    _same(open(depth).read(), pk.depth_lines(pu, g.frag_start, g.frag_names), "-pileup_depth")
    assert ("pileup gapped: file=%s placements=%d ungapped=%d aligned=%d " % (fa, pu.gstats["placed"], pu.gstats["ungapped"], pu.gstats["aligned_bases"])) in r.stderr.decode()
    r = cli._run(base + ["-o", out, "-vcf", vf, "-pileup_gapped", "1"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    _same(open(vf).read(), ck.vcf_header(vcf_cli._contigs([g])) + ck.vcf_lines(cl.calls(), g.frag_start, names), "-vcf")
    assert (pgc.stderr_line(pu, fa) + "\n") in r.stderr.decode()
    assert cl.calls().shape[0] >= 10 and (ck.stderr_line(cl, fa) + "\n") in r.stderr.decode()


def test_real_cli_pileup_gapped_loud_refusals(tmp_path):
    g = synth.random_genome(60_000, seed=7)
    b1, b2 = synth.sample_pairs(g, 50, 100, 100, 300, 30, 0.0, 8)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    out, sites = str(tmp_path / "out.tsv"), str(tmp_path / "s.tsv")
    base = [cli.REAL, "-t", fa, "-o", out, "-Q", "33", "-insert_min", "150", "-insert_max", "420", "-p", p1]
    ok = cli._run(base + ["-p2", p2, "-pileup", sites, "-pileup_gapped", "1"])
    assert ok.returncode == 0 and b"pileup gapped: file=" in ok.stderr and b"placements=0" in ok.stderr
    for args, word in ((["-pileup", sites, "-pileup_gapped", "1"], b"single-end drivers are not there yet"),
                       (["-p2", p2, "-pileup_gapped", "1"], b"needs one of -pileup / -pileup_depth / -vcf"),
                       (["-p2", p2, "-pileup", sites, "-pileup_gapped", "1", "-pairs_all", "1"], b"-pairs_all"),
                       (["-p2", p2, "-pileup", sites, "-pileup_gapped"], b"missing")):
        r = cli._run(base + args)
        assert r.returncode != 0 and word in r.stderr and b"Processing file" not in r.stderr, (args, r.stderr.decode()[-500:])
