"""End-to-end: `real -p mates1 -p2 mates2 -mate_search 1` against lines built from the checker's records
(mate_search_checker.py); without the flag the output is what the paired-end mode gave before."""
import pytest

import mate_search_checker as mc
import mate_search_workloads as mw
import pairs_checker as pc
import test_cli_pairs_gpu as cli
from real_amd import synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scores,extra,max_anchors", [(1, [], 0), (0, ["-batch", "400"], 0), (1, ["-mate_search_anchors", "4"], 4)])
def test_real_cli_mate_search(ora, tmp_path, scores, extra, max_anchors):
    g, b1, b2, _ = mw.search_workload("families", True, (100, 80), 32, 3)
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    base = [cli.REAL, "-t", fa, "-p", p1, "-p2", p2, "-insert_min", str(mw.MIN_INS), "-insert_max", str(mw.MAX_INS), "-e", "3", "-s", "2", "-l", "32",
            "-q", str(scores)]
    f = mw.oracle_lists(ora, g, b1, b2, 32, 3, scores, 2)
    args = (b1, b2, mw.MIN_INS, mw.MAX_INS, scores, ora.filter_mult(2, 3), 32, 3)
    off, _ = mc.check_pairs_search(ora, {0: g}, [f], *args, search=False)
    on, _ = mc.check_pairs_search(ora, {0: g}, [f], *args, max_anchors=max_anchors)
    out = {}
    for name, flags in (("off", []), ("zero", ["-mate_search", "0"]), ("on", ["-mate_search", "1"] + extra)):
        path = str(tmp_path / (name + ".tsv"))
        r = cli._run(base + ["-o", path] + flags)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out[name] = open(path, "rb").read()
    want_off = cli.expected_lines(off, [g], b1, b2, scores)
    want_on = cli.expected_lines(on, [g], b1, b2, scores)
    assert out["off"] == out["zero"] and out["off"].decode().split("\n")[:-1] == want_off      # byte-identical without the flag
    assert out["on"].decode().split("\n")[:-1] == want_on
    assert want_on != want_off and len(want_on) > 400
    assert (off["state"] != on["state"]).sum() >= 20


def test_real_cli_mate_search_150bp_seed_64(ora, tmp_path):
    """2 x 150 bases, 64-base seeds, five mismatches, inserts 200..700, random qualities"""
    row = mw.PROTOCOL_ROWS[0]
    assert (row.patl, row.seedl, row.tk, row.min_ins, row.max_ins) == ((150, 150), 64, 5, 200, 700)
    g, b1, b2, _ = mw.protocol_search_workload(row, "iid")
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    p1, p2 = cli._write(tmp_path, b1, b2)
    base = [cli.REAL, "-l", "64", "-e", "5", "-t", fa, "-p", p1, "-p2", p2, "-insert_min", "200", "-insert_max", "700", "-s", "2", "-q", "1", "-Q", "33"]
    f = mw.oracle_lists(ora, g, b1, b2, 64, 5, 1, 2)
    args = (b1, b2, 200, 700, 1, ora.filter_mult(2, 5), 64, 5)
    off, _ = mc.check_pairs_search(ora, {0: g}, [f], *args, search=False)
    on, _ = mc.check_pairs_search(ora, {0: g}, [f], *args)
    out = {}
    for name, flags in (("off", []), ("on", ["-mate_search", "1"])):
        path = str(tmp_path / (name + ".tsv"))
        r = cli._run(base + ["-o", path] + flags)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out[name] = open(path, "rb").read()
    want_off = cli.expected_lines(off, [g], b1, b2, 1)
    want_on = cli.expected_lines(on, [g], b1, b2, 1)
    assert out["off"].decode().split("\n")[:-1] == want_off
    assert out["on"].decode().split("\n")[:-1] == want_on
    assert want_on != want_off and len(want_on) > 100
    assert (off["state"] != on["state"]).sum() >= 20
