"""End-to-end at the edges of the batch domain: `real -sam -pileup` on a FASTQ of 100-base reads with reads of 2048, 2049 and
16384 bases and a record without bases among them, quality characters up to '~' (offset 33, detected from the file), parsed on
the device and by the host reader.  Both runs write the same bytes; the lines are the oracle's, QUAL is the input's quality
line (reversed on the reverse strand), NM the oracle's error count.  A read of 16385 bases ends the run before any output."""
import os
import subprocess

import numpy as np
import pytest

import domain_workloads as dw
import pileup_checker as pk
import sam_checker as sk
import test_cli_gpu as cli1
from real_amd import synth

pytestmark = pytest.mark.gpu
MATCH = ["-e", str(dw.TOTALKMAX), "-s", str(dw.SEEDKMAX), "-l", "32", "-q", "1"]
LONG = (2048, 2049, 16384)
TOP = ord("~") - 33


def _reads():
    """60 reads of 100 bases; per long length the read with totalkmax substitutions and the mid-text read of the reverse strand;
    one record without bases.  Qualities 0..93; the file's first quality character is '!', which makes the offset 33"""
    w = dw.workload()
    rng = np.random.default_rng(77)
    fill = synth.sample_reads(w.g, 60, 100, 0.02, seed=78, n_read_prob=0.001)
    reads = [(fill.bases[100 * i:100 * i + 100], "fill%d" % i) for i in range(60)]
    for L in LONG:
        for kind, inv in (("kmax", 0), ("mid", 1)):
            i = dw.index_of(w, L, kind, inv)
            reads.insert(7 * len(reads) // 11, (w.b.bases[int(w.b.offsets[i]):int(w.b.offsets[i + 1])], "%s%d_L%d" % (kind, inv, L)))
    reads.insert(20, (np.zeros(0, np.uint8), "nothing"))
    b = synth.ReadBatch(bases=np.concatenate([r[0] for r in reads]).astype(np.uint8), qual=None,
                        offsets=np.cumsum([0] + [r[0].shape[0] for r in reads]).astype(np.uint64), ids=[r[1] for r in reads])
    b.qual = rng.integers(0, TOP + 1, size=b.bases.shape[0]).astype(np.uint8)
    for i in range(b.n_reads):
        lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
        if hi > lo:
            b.qual[lo], b.qual[hi - 1] = (0 if i == 0 else TOP), TOP
    return w.g, b


def _run(cmd):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_real_cli_on_long_reads_an_empty_record_and_qualities_up_to_tilde(ora, tmp_path):
    g, b = _reads()
    assert int(b.qual.max()) == 93 and b.qual[0] == 0
    fa, rd = cli1.write_inputs(tmp_path, g, b)
    qlines = open(rd).read().split("\n")[3::4]
    assert max(max(q) for q in qlines if q) == "~" and "" in qlines
    outs = {}
    for parse in ("1", "0"):
        names = [str(tmp_path / ("%s.%s" % (k, parse))) for k in ("tsv", "sam", "pileup")]
        r = _run([cli1.REAL, "-t", fa, "-p", rd, "-o", names[0], "-sam", names[1], "-pileup", names[2], "-gpuparse", parse] + MATCH)
        assert r.returncode == 0, r.stderr.decode()[-2000:]          # (nothing more is started behind a run that failed)
        assert parse == "0" or b"host reader takes over" not in r.stderr, r.stderr.decode()[-1500:]
        outs[parse] = [open(n).read() for n in names]
    for k, a, c in zip(("tsv", "sam", "pileup"), outs["1"], outs["0"]):
        assert a == c, k
    tsv, sam, pile = outs["1"]
    info, score = cli1.oracle_unique(ora, g, b, 32, dw.SEEDKMAX, dw.TOTALKMAX, 1)
    want = cli1.expected_unique(ora, g, b, info, score, 1)
    assert tsv.split("\n")[:-1] == want
    st, _, er, _, _ = ora.unpack_record(info)
    by_id = {b.ids[i]: i for i in range(b.n_reads)}
    for L in LONG:
        assert st[by_id["kmax0_L%d" % L]] == 1 and er[by_id["kmax0_L%d" % L]] == dw.TOTALKMAX and st[by_id["mid1_L%d" % L]] == 2
    seen = 0
    for line in sam.split("\n")[:-1]:
        if line.startswith("@"):
            continue
        f = line.split("\t")
        i = by_id[f[0]]
        seen += 1
        placed = st[i] in (1, 2)
        assert int(f[1]) == (16 if st[i] == 2 else 0 if placed else 4), line[:80]
        if f[0] == "nothing":
            continue
        q = qlines[i]
        assert f[10] == (q[::-1] if st[i] == 2 else q), f[0]
        if placed:
            assert ("NM:i:%d" % er[i]) in f[11:], (f[0], f[11:])
    assert seen == b.n_reads
    want_sam, stats = sk.sam_single([g], b, info, score, True)
    skip = lambda text: [x for x in text.split("\n") if not x.startswith("nothing\t")]
    assert skip(sam) == skip(want_sam)
    assert stats[0]["disagree"] == 0 and stats[0]["placed"] >= 35
    pu = pk.Pileup(g.sym, 0, 0)
    pu.add(b, info)
    assert pile == pk.pileup_lines(pu, g.frag_start, g.frag_names) and pu.sites().shape[0] >= 3 * dw.TOTALKMAX


@pytest.mark.parametrize("parse", ["1", "0"])
def test_real_cli_refuses_a_read_of_16385_bases(tmp_path, parse):
    g, b = _reads()
    w = dw.workload()
    more = synth.ReadBatch(bases=w.g.sym[dw.P_MID:dw.P_MID + 16385].copy(), qual=np.full(16385, 40, np.uint8),
                           offsets=np.array([0, 16385], dtype=np.uint64), ids=["too_long"])
    fa, rd = cli1.write_inputs(tmp_path, g, synth.concat_batches([b, more]))
    out = str(tmp_path / "out.tsv")
    r = _run([cli1.REAL, "-t", fa, "-p", rd, "-o", out, "-gpuparse", parse] + MATCH)
    err = r.stderr.decode()
    assert r.returncode != 0 and ("16384" in err or "REAL_HIP_MAX_PATL_LONG" in err), err[-1500:]
    assert not os.path.exists(out) or os.path.getsize(out) == 0
