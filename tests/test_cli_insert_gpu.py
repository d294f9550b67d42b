"""End-to-end: `real -p mates1 -p2 mates2 -insert_auto N` and `-insert_hist <file>`.  The estimated bounds are the checker's
(insert_checker.py over the checker's pair records of the oracle's match_all lists), the run that follows is byte for byte
the run with those bounds given, and the histogram file and its quartiles are the checker's on the final records."""
import re

import numpy as np
import pytest

import insert_checker as ic
import insert_workloads as iw
import pairs_checker as pc
import pairs_workloads as pw
import test_cli_pairs_gpu as cli
from real_amd import lib as rlib
from real_amd import synth

pytestmark = pytest.mark.gpu
AUTO, BATCH = 600, 400             # the probe takes a whole batch and a partial one


def _base(tmp_path, g, b1, b2, fa=None):
    if fa is None:
        fa = str(tmp_path / "genome.fa")
        synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    return [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-e", str(iw.TOTALK), "-s", "2", "-l", str(iw.SEEDL), "-q", "1"]


@pytest.mark.parametrize("kind,ragged,search", [("iid", True, False), ("families", False, False), ("families", False, True)])
def test_real_cli_insert_auto(ora, tmp_path, kind, ragged, search):
    g, b1, b2 = iw.workload(kind, ragged)
    base = _base(tmp_path, g, b1, b2) + (["-mate_search", "1"] if search else [])
    lo, hi = iw.WINDOW
    window = ["-insert_min", str(lo), "-insert_max", str(hi)]
    auto, given = str(tmp_path / "auto.tsv"), str(tmp_path / "given.tsv")
    r = cli._run(base + window + ["-o", auto, "-insert_auto", str(AUTO), "-batch", str(BATCH)])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    line = re.search(r"^insert size estimate: fragments=(\d+) unique=(\d+) q1=(\d+) median=(\d+) q3=(\d+) bounds=\[(\d+), (\d+)\]$", r.stderr.decode(), re.M)
    assert line, r.stderr.decode()[-2000:]
    got = [int(x) for x in line.groups()]
    a, b = got[5], got[6]
    # the checker's records of the first 600 fragments under the window (with the search: the placements it adds count too)
    rec, l1, l2 = iw.records_with_search(ora, kind, ragged, 1, AUTO) if search else iw.records(ora, kind, ragged, 1, n=AUTO)
    rc, est, want = iw.sample_bounds(rec, l1, l2)
    assert rc == 0 and got == [AUTO, est["n"], est["q1"], est["median"], est["q3"], want[0], want[1]], (got, est, want)
    assert lo < a < 250 and 350 < b < hi, (a, b)         # the library's mean is 300: the bounds cut the window on both sides
    r2 = cli._run(base + ["-o", given, "-insert_min", str(a), "-insert_max", str(b), "-batch", str(BATCH)])
    assert r2.returncode == 0 and b"insert size estimate" not in r2.stderr
    out = open(auto, "rb").read()
    assert len(out.split(b"\n")) > 1500 and out == open(given, "rb").read()


def _two_files(tmp_path):
    g0 = synth.random_genome(150_000, seed=501, n_frag=2)
    g1 = synth.random_genome(120_000, seed=502, n_frag=3)
    g1.sym[1000:2600] = g0.sym[1000:2600]
    pa = synth.sample_pairs(g0, 400, 100, 100, 300, 30, 0.02, 61, insert_min=150, insert_max=420)
    pb = synth.sample_pairs(g1, 300, 100, 80, 300, 30, 0.02, 62, insert_min=150, insert_max=420)
    shared = synth.Genome(sym=g0.sym[1000:2600].copy(), frag_start=np.array([0, 1600], dtype=np.uint64))
    ps = synth.sample_pairs(shared, 100, 100, 100, 300, 30, 0.0, 63, insert_min=150, insert_max=420, straddle_frac=0)
    b1 = synth.concat_batches([pa[0], pb[0], ps[0]])
    b2 = synth.concat_batches([pa[1], pb[1], ps[1]])
    d = tmp_path / "genomes"
    d.mkdir()
    synth.genome_to_fasta(g0, str(d / "a.fa"))
    synth.genome_to_fasta(g1, str(d / "b.fa"))
    return {"a": g0, "b": g1}, b1, b2, str(d)


def test_real_cli_insert_hist_two_genome_files(ora, tmp_path):
    """the histogram is taken from the FINAL records: the fragments of the stretch both files hold are NonUnique and count nowhere"""
    by_name, b1, b2, d = _two_files(tmp_path)
    base = _base(tmp_path, None, b1, b2, fa=d) + ["-insert_min", "150", "-insert_max", "420", "-batch", "300"]
    out, plain, hf = str(tmp_path / "out.tsv"), str(tmp_path / "plain.tsv"), str(tmp_path / "hist.tsv")
    r0 = cli._run(base + ["-o", plain])
    r = cli._run(base + ["-o", out, "-insert_hist", hf])
    assert r0.returncode == 0 and r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out, "rb").read() == open(plain, "rb").read() and b"insert size" not in r0.stderr
    order = re.findall(r"Processing file \S*/([ab])\.fa", r.stderr.decode())     # the file ids follow the directory's own order
    assert sorted(order) == ["a", "b"]
    genomes = [by_name[x] for x in order]
    files = [pw.oracle_pairs(ora, g, b1, b2, iw.SEEDL, iw.TOTALK, 1, iw.FILTER_LEVEL, fileid=fid)[0] for fid, g in enumerate(genomes)]
    l1, l2 = pw.lens_of(b1), pw.lens_of(b2)
    rec = pc.check_pairs(files, l1, l2, 150, 420, 1, ora.filter_mult(iw.FILTER_LEVEL, iw.TOTALK))
    assert open(out).read().split("\n")[:-1] == cli.expected_lines(rec, genomes, b1, b2, 1)
    want, wst = ic.histogram(rec, l1, l2, 422)
    assert wst["counted"] == int((rec["state"] == pc.UNIQUE).sum()) > 400 and wst["overflow"] == 0 and wst["invalid"] == 0
    assert (rec["state"][700:800] == pc.NONUNIQUE).sum() >= 90
    lines = open(hf).read().split("\n")
    assert lines[-1] == "" and lines[:-1] == ["%d\t%d" % (x, want[x]) for x in np.nonzero(want)[0]]
    rc, est = ic.bounds(want)
    assert rc == 0 and ("insert size: n=%d q1=%d median=%d q3=%d\n" % (est["n"], est["q1"], est["median"], est["q3"])) in r.stderr.decode()
    # with -insert_auto in front: the histogram has the bins of the bounds in force
    r = cli._run(base + ["-o", out, "-insert_hist", hf, "-insert_auto", "500"])
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    a, b = (int(x) for x in re.search(r"bounds=\[(\d+), (\d+)\]", r.stderr.decode()).groups())
    rec = pc.check_pairs(files, l1, l2, a, b, 1, ora.filter_mult(iw.FILTER_LEVEL, iw.TOTALK))
    want, _ = ic.histogram(rec, l1, l2, b + 2)
    assert 150 <= a and b <= 420 and open(hf).read().split("\n")[:-1] == ["%d\t%d" % (x, want[x]) for x in np.nonzero(want)[0]]


def test_real_cli_insert_loud_errors(tmp_path):
    g = synth.random_genome(60_000, seed=7)
    b1, b2 = synth.sample_pairs(g, 50, 100, 100, 300, 30, 0.0, 8)
    base = _base(tmp_path, g, b1, b2) + ["-Q", "33"]
    out, u, hf = str(tmp_path / "out.tsv"), str(tmp_path / "u.tsv"), str(tmp_path / "hist.tsv")
    nop2 = base[:base.index("-p2")] + base[base.index("-p2") + 2:] + ["-o", out]
    base = base + ["-o", out]
    r = cli._run(base + ["-insert_hist", hf, "-insert_auto", "5000"])       # fewer fragments than N: the estimate takes what there is
    assert r.returncode == 0 and b"insert size estimate: fragments=50 " in r.stderr and b"insert size: n=" in r.stderr, r.stderr.decode()[-2000:]
    top = rlib.REAL_HIP_INSERT_HIST_MAX_BINS - 2
    for args, word in ((nop2 + ["-insert_hist", hf], b"-p2"), (nop2 + ["-insert_auto", "50"], b"-p2"),
                       (base + ["-insert_hist", hf, "-pairs_all", "1"], b"-pairs_all"), (base + ["-insert_auto", "50", "-pairs_all", "1"], b"-pairs_all"),
                       (base + ["-insert_hist", hf, "-insert_max", str(top + 1)], b"-insert_max"),
                       (base + ["-insert_auto", "50", "-insert_max", str(top + 1)], b"-insert_max"),
                       (base + ["-insert_hist", out], b"same file as -o"), (base + ["-insert_hist", u, "-unpaired", u], b"same file as -unpaired"),
                       # too few unique fragments in the sample; a window the library does not fit into (no unique fragment at all)
                       (base + ["-insert_auto", "20"], b"give the bounds explicitly"),
                       (base + ["-insert_auto", "50", "-insert_min", "0", "-insert_max", "120"], b"give the bounds explicitly")):
        r = cli._run(args)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr.decode()[-500:])
