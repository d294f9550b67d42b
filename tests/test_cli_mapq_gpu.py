"""End-to-end: `real -mapq 1` with -sam, and -pileup_minmapq, single-end and with -p2.  The SAM file of the run with the flag is
the run's without it in every column but MAPQ, which is the checker's (mapq_checker.py over the oracle's lists and final
records); -o is byte for byte the same; the pileup under -pileup_minmapq Q is the pileup checker's over the records with the
placements below Q masked.  Child processes only, each under its own time limit."""
import re

import numpy as np
import pytest

import mapq_checker as mq
import mapq_workloads as mqw
import mate_search_checker as mc
import mate_search_workloads as msw
import pairs_checker as pc
import pileup_checker as pk
import pileup_workloads as pw
import singles_checker as sc
import test_cli_gpu as cli1
import test_cli_pairs_gpu as cli
from real_amd import synth

pytestmark = pytest.mark.gpu
Q, Q_PAIRS = 30, 40        # on mapq_workloads.near_copy_workload: a fifth of the placed reads lie below 30, 30 Unique fragments below 40


def _run(cmd):
    r = cli._run(cmd)
    assert r.returncode == 0, r.stderr.decode()[-2000:]          # (nothing more is started behind a run that failed)
    return r.stderr.decode()


def _sam_lines(path):
    return [l.split("\t") for l in open(path).read().split("\n")[:-1] if not l.startswith("@")]


def _same_but_mapq(plain, with_mapq):
    """every header line and every column but MAPQ; without the flag MAPQ is 255 on the placed reads -> the MAPQ column of the second"""
    a, b = open(plain).read().split("\n"), open(with_mapq).read().split("\n")
    assert len(a) == len(b) and len(a) > 500
    col = []
    for x, y in zip(a, b):
        if x.startswith("@") or not x:
            assert x == y
            continue
        x, y = x.split("\t"), y.split("\t")
        assert x[:4] == y[:4] and x[5:] == y[5:], (x, y)
        assert x[4] == ("0" if int(x[1]) & 4 else "255")
        col.append(int(y[4]))
    return col


def _mapq_line(err):
    m = re.findall(r"^mapq: placements=(\d+) unlisted=(\d+) mean=([0-9.]+)$", err, re.M)
    assert len(m) == 1, err[-1500:]
    return int(m[0][0]), int(m[0][1]), m[0][2]


def _names(g):
    return g.frag_names if g.frag_names else [" frag%d" % k for k in range(g.n_frag)]


_single = {}


def _single_end(ora):
    """the single-end reads of the near-copy workload: (genome, reads, oracle records, the checker's qualities, placements, unlisted)"""
    if not _single:
        g, b, _, _ = mqw.near_copy_workload()
        info, score = cli1.oracle_unique(ora, g, b, mqw.NC_SEEDL, 2, mqw.NC_TOTALK, 1)
        og = ora.Genome(g.sym, g.frag_start)
        p = ora.make_params(seedl=mqw.NC_SEEDL, seedkmax=2, totalkmax=mqw.NC_TOTALK, scores=1, filter_level=2, fileid=0)
        h, o, _ = ora.match_all(og, ora.Index(og, mqw.NC_SEEDL), p, b.bases, b.qual, b.offsets)
        state, _, err, _, _ = ora.unpack_record(info)
        _single["x"] = (g, b, info, score) + mq.finish_single(state, err, score, mq.check_hits([(h, o)], b.n_reads, 1), 1)
    return _single["x"]


def _match_flags():
    return ["-e", str(mqw.NC_TOTALK), "-s", "2", "-l", str(mqw.NC_SEEDL), "-q", "1", "-Q", "33"]


def test_real_cli_mapq_single_end(ora, tmp_path):
    g, b, info, score, want, placed, unl = _single_end(ora)
    fa, rd = cli1.write_inputs(tmp_path, g, b)
    f = {k: str(tmp_path / k) for k in ("o0", "s0", "p0", "o1", "s1", "p1")}
    base = [cli.REAL, "-t", fa, "-p", rd, "-batch", "700", "-gpuparse", "0"] + _match_flags()
    e0 = _run(base + ["-o", f["o0"], "-sam", f["s0"], "-pileup", f["p0"]])
    e1 = _run(base + ["-o", f["o1"], "-sam", f["s1"], "-pileup", f["p1"], "-mapq", "1", "-pileup_minmapq", "0"])
    assert "mapq:" not in e0 and open(f["o0"], "rb").read() == open(f["o1"], "rb").read()
    assert open(f["o1"]).read().split("\n")[:-1] == cli1.expected_unique(ora, g, b, info, score, 1)
    assert open(f["p0"], "rb").read() == open(f["p1"], "rb").read() and len(open(f["p0"], "rb").read()) > 1000       # Q = 0 masks nothing
    col = _same_but_mapq(f["s0"], f["s1"])                  # one genome file: the lines are in read order
    lines = _sam_lines(f["s1"])
    assert len(col) == b.n_reads and [int(l[1]) & 4 for l in lines] == [4 * int(q == mq.NONE) for q in want]
    assert col == [0 if q == mq.NONE else int(q) for q in want]
    vals = sorted(set(int(q) for q in want) - {mq.NONE})
    assert len(vals) >= 10 and vals[-1] == 60 and sum(q < 60 for q in want) > 200, vals       # (the near copies: 25 values, 252 reads below 60)
    assert _mapq_line(e1) == (placed, unl, "%.3f" % (sum(int(q) for q in want if q != mq.NONE) / placed)) and unl == 0
    assert e1.replace(re.search(r"^mapq:.*\n", e1, re.M).group(0), "").count("sam:") == e0.count("sam:") == 1
    assert re.findall(r"^sam:.*$", e0, re.M) == re.findall(r"^sam:.*$", e1, re.M)


def test_real_cli_pileup_minmapq_single_end(ora, tmp_path):
    g, b, info, score, want, _, _ = _single_end(ora)
    fa, rd = cli1.write_inputs(tmp_path, g, b)
    out, pf, df, vf = (str(tmp_path / k) for k in ("out.tsv", "pileup.tsv", "depth.tsv", "calls.vcf"))
    err = _run([cli.REAL, "-t", fa, "-p", rd, "-o", out, "-pileup", pf, "-pileup_depth", df, "-vcf", vf, "-mapq", "1", "-pileup_minmapq", str(Q)] + _match_flags())
    assert open(out).read().split("\n")[:-1] == cli1.expected_unique(ora, g, b, info, score, 1)                # -o does not change
    below = (want != mq.NONE) & (want < Q)
    masked = np.where(below, np.uint64(0), info)
    assert below.sum() >= 100 and ((want != mq.NONE) & ~below).sum() > 400
    pu, whole = pk.Pileup(g.sym, 0, 0), pk.Pileup(g.sym, 0, 0)
    pu.add(b, masked)
    whole.add(b, info)
    assert pu.stats["placed"] == whole.stats["placed"] - int(below.sum())
    assert open(pf).read() == pk.pileup_lines(pu, g.frag_start, _names(g)) != pk.pileup_lines(whole, g.frag_start, _names(g))
    assert open(df).read() == pk.depth_lines(pu, g.frag_start, _names(g))
    assert (pk.stderr_line(pu, fa) + "\n") in err, err[-1500:]
    assert ("calls: file=%s sites=%d " % (fa, pu.finish_stats()["sites"])) in err                             # the calls sit on the masked pileup


def test_real_cli_mapq_two_genome_files(ora, tmp_path):
    """the accumulators fold over both files as the records do: a read with a copy in each file is rated against both"""
    w = pw.workload()
    g2, b2 = pw.second_genome()
    g2.sym[3000:4200] = w.g.sym[40_000:41_200]                       # a stretch both files hold, the second with a substitution every 100 bases,
    g2.sym[3025:4200:100] = (g2.sym[3025:4200:100] + 1) & 3          # and reads from the first: Unique there, and rated against the copy
    rng = np.random.default_rng(9)
    from pileup_workloads import _sample
    shared = _sample(rng, w.g.sym, [(40_000 + int(rng.integers(0, 1000)), 100, bool(i & 1)) for i in range(60)], 0.02, "x")
    by_name = {"a": w.g, "b": g2}
    d = tmp_path / "genomes"
    d.mkdir()
    synth.genome_to_fasta(w.g, str(d / "a.fa"))
    synth.genome_to_fasta(g2, str(d / "b.fa"))
    reads = synth.concat_batches([w.main, b2, shared])
    rd = str(tmp_path / "reads.fq")
    synth.reads_to_fastq(reads, rd)
    f = {k: str(tmp_path / k) for k in ("o0", "s0", "o1", "s1")}
    base = [cli.REAL, "-t", str(d), "-p", rd, "-batch", "700", "-gpuparse", "0", "-e", "3", "-s", str(pw.SEEDK), "-l", str(pw.SEEDL), "-q", "1", "-Q", "33"]
    _run(base + ["-o", f["o0"], "-sam", f["s0"]])          # (-e 3: eps is 4.3 bits of the window's 15.5; the workload's own -e 10 leaves 1.2)
    err = _run(base + ["-o", f["o1"], "-sam", f["s1"], "-mapq", "1"])
    assert open(f["o0"], "rb").read() == open(f["o1"], "rb").read()
    order = re.findall(r"Processing file (\S*/([ab])\.fa)", err)         # the file ids follow the directory's own order
    assert sorted(x[1] for x in order) == ["a", "b"]
    info, score, blocks = None, None, []
    for fid, (_, name) in enumerate(order):
        g = by_name[name]
        og = ora.Genome(g.sym, g.frag_start)
        p = ora.make_params(seedl=pw.SEEDL, seedkmax=pw.SEEDK, totalkmax=3, scores=1, filter_level=pw.FILTER_LEVEL, fileid=fid)
        ix = ora.Index(og, pw.SEEDL)
        info, score, _ = ora.match_unique(og, ix, p, reads.bases, reads.qual, reads.offsets, info=info, score=score)
        h, o, _ = ora.match_all(og, ix, p, reads.bases, reads.qual, reads.offsets)
        blocks.append((h, o))
    accs = mq.check_hits(blocks, reads.n_reads, 1)
    state, _, errors, _, _ = ora.unpack_record(info)
    want, placed, unl = mq.finish_single(state, errors, score, accs, 1)
    col = _same_but_mapq(f["s0"], f["s1"])
    by_id = {}
    for l, q in zip(_sam_lines(f["s1"]), col):
        assert l[0] not in by_id
        by_id[l[0]] = q
    assert [by_id[reads.ids[i].split()[0]] for i in range(reads.n_reads)] == [0 if q == mq.NONE else int(q) for q in want]
    both = sum(1 for i in range(reads.n_reads) if blocks[0][1][i + 1] > blocks[0][1][i] and blocks[1][1][i + 1] > blocks[1][1][i])
    assert both >= 40 and sum(q < 60 for q in want) >= 10 and _mapq_line(err)[:2] == (placed, unl)      # (below 60 through the other file's copy)


def _pair_flags(min_ins, max_ins):
    return ["-insert_min", str(min_ins), "-insert_max", str(max_ins)] + _match_flags()


def test_real_cli_mapq_pairs_and_pileup_minmapq(ora, tmp_path):
    """-p2: both mates of a Unique fragment carry the fragment's quality, a mate placed on its own its own; the pileup leaves out
    the fragments below Q"""
    g, _, b1, b2 = mqw.near_copy_workload()
    lo, hi = mqw.NC_INS
    lists = msw.oracle_lists(ora, g, b1, b2, mqw.NC_SEEDL, mqw.NC_TOTALK, 1, 2)
    _, h1, o1, h2, o2 = lists
    l1, l2, fm = msw.lens_of(b1), msw.lens_of(b2), ora.filter_mult(2, mqw.NC_TOTALK)
    rec = pc.check_pairs([lists], l1, l2, lo, hi, 1, fm)
    s1, s2 = sc.check_singles([(0, h1, o1)], l1, 1, fm), sc.check_singles([(0, h2, o2)], l2, 1, fm)
    want, placed, unl = mq.finish_pairs(rec, s1, s2, mq.check_pair_hits([(h1, o1, h2, o2)], l1, l2, lo, hi, 1), mq.check_hits([(h1, o1)], len(l1), 1),
                                        mq.check_hits([(h2, o2)], len(l2), 1), 1)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    f = {k: str(tmp_path / k) for k in ("o0", "s0", "o1", "s1", "p1")}
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-batch", "500"] + _pair_flags(lo, hi)
    _run(base + ["-o", f["o0"], "-sam", f["s0"]])
    err = _run(base + ["-o", f["o1"], "-sam", f["s1"], "-mapq", "1", "-pileup", f["p1"], "-pileup_minmapq", str(Q_PAIRS)])
    assert open(f["o0"], "rb").read() == open(f["o1"], "rb").read()
    assert open(f["o1"]).read().split("\n")[:-1] == cli.expected_lines(rec, [g], b1, b2, 1)
    col = _same_but_mapq(f["s0"], f["s1"])                  # one genome file: mate 1, mate 2 of every fragment in read order
    assert col == [0 if q == mq.NONE else int(q) for q in want]
    assert _mapq_line(err)[:2] == (placed, 0) and unl == 0
    unique = rec["state"] == 1
    assert (want[0::2] == want[1::2])[unique].all() and len(set(int(q) for q in want[0::2][unique])) >= 8 and ((want[0::2] != want[1::2]) & ~unique).sum() >= 20
    below = unique & (want[0::2] < Q_PAIRS)
    masked = rec.copy()
    masked["state"][below] = 0
    assert below.sum() >= 20 and (unique & ~below).sum() > 500
    pu = pk.Pileup(g.sym, 0, 0)
    pu.add_pairs(b1, b2, masked)
    assert open(f["p1"]).read() == pk.pileup_lines(pu, g.frag_start, _names(g))
    assert (pk.stderr_line(pu, fa) + "\n") in err, err[-1500:]


def test_real_cli_mapq_pairs_with_the_mate_search(ora, tmp_path):
    """-mate_search 1: the placements only the search found are rated as unlisted"""
    scores, tk, fl, seedl = 1, 3, 2, 32
    g, b1, b2, planted = msw.search_workload("iid", False, (100, 80), seedl, tk)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    f = {k: str(tmp_path / k) for k in ("o0", "s0", "o1", "s1")}
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-insert_min", str(msw.MIN_INS), "-insert_max", str(msw.MAX_INS), "-e", "3", "-s", "2", "-l", "32",
            "-q", "1", "-mate_search", "1"]
    _run(base + ["-o", f["o0"], "-sam", f["s0"]])
    err = _run(base + ["-o", f["o1"], "-sam", f["s1"], "-mapq", "1"])
    assert open(f["o0"], "rb").read() == open(f["o1"], "rb").read()
    lists = msw.oracle_lists(ora, g, b1, b2, seedl, tk, scores, fl)
    fm = ora.filter_mult(fl, tk)
    on, _ = mc.check_pairs_search(ora, {0: g}, [lists], b1, b2, msw.MIN_INS, msw.MAX_INS, scores, fm, seedl, tk)
    _, h1, o1, h2, o2 = lists
    l1, l2 = msw.lens_of(b1), msw.lens_of(b2)
    s1, s2 = sc.check_singles([(0, h1, o1)], l1, scores, fm), sc.check_singles([(0, h2, o2)], l2, scores, fm)
    accp = mq.check_pair_hits([(h1, o1, h2, o2)], l1, l2, msw.MIN_INS, msw.MAX_INS, scores)
    want, placed, unl = mq.finish_pairs(on, s1, s2, accp, mq.check_hits([(h1, o1)], len(l1), scores), mq.check_hits([(h2, o2)], len(l2), scores), scores)
    col = _same_but_mapq(f["s0"], f["s1"])
    assert col == [0 if q == mq.NONE else int(q) for q in want]
    assert unl >= 8 and _mapq_line(err)[:2] == (placed, unl)
