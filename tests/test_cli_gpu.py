"""End-to-end: the `real` command line (real_amd/host/real, C++ over the C ABI) against the
11-column output the reference's printMatchUnlocked would write for the oracle's records
(matchUniqueImplementation.cpp:252-321; matchAll: matchAllImplementation.cpp:481-518)."""
import os
import subprocess

import numpy as np
import pytest

from real_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REAL = os.path.join(ROOT, "real_amd", "host", "real")


def fmt_float(x):
    return "%g" % float(np.float32(x))          # ostream << float: 6 significant digits


def seq(bases, inverted):
    b = synth.revcomp(bases) if inverted else bases
    return "".join("ACGTN"[c] for c in b)


def expected_unique(ora, g, b, info, score, scores):
    st, fr, er, fi, po = ora.unpack_record(info)
    lines = []
    for i in range(b.n_reads):
        if st[i] not in (1, 2):
            continue
        lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
        lines.append("\t".join([b.ids[i], seq(b.bases[lo:hi], st[i] == 2), fmt_float(score[i]) if scores else "", "1", "a",
                                str(hi - lo), "-" if st[i] == 2 else "+", g.frag_names[fr[i]],
                                str(po[i] - int(g.frag_start[fr[i]]) + 1), "", str(er[i])]))
    return lines


def write_inputs(tmp_path, g, b, fastq=True):
    fa = str(tmp_path / "genome.fa")
    synth.genome_to_fasta(g, fa)
    rd = str(tmp_path / ("reads.fq" if fastq else "reads.fa"))
    (synth.reads_to_fastq if fastq else synth.reads_to_fasta)(b, rd)
    return fa, rd


def oracle_unique(ora, g, b, seedl, seedk, totalk, scores, n_list=0, fasta=False):
    og = ora.Genome(g.sym, g.frag_start)
    p = ora.make_params(seedl=seedl, seedkmax=seedk, totalkmax=totalk, scores=scores)
    qual = np.full_like(b.qual, 30) if fasta else b.qual
    info = np.zeros(b.n_reads, np.uint64)
    score = np.full(b.n_reads, ora.NOSCORE_INIT, np.float32)
    first = 0
    while True:
        ix = ora.Index(og, seedl, first, n_list if n_list else 1 << 62)
        info, score, _ = ora.match_unique(og, ix, p, b.bases, qual, b.offsets, info=info, score=score)
        first += ix.n
        if not ix.have_next:
            break
    return info, score


@pytest.mark.parametrize("scores,extra,n_list,fastq", [
    (1, [], 0, True),
    (0, [], 0, True),
    (1, ["-index", "host", "-T", "3"], 0, True),
    (1, ["-block", "30000", "-batch", "500"], 30000, True),      # three index blocks, several read batches
    (1, [], 0, False),                                             # FASTA reads: constant quality 30
    (1, ["-gpuparse", "0"], 0, True),                              # read file parsed by the host reader
    (1, ["-table_kind", "3", "-l", "16", "-prefix_bits", "13"], 0, True),   # bucket rows (seed length 16 so that they are small)
    (1, ["-wrap"], 0, False),                                      # wrapped FASTA: the device parser refuses, host reader takes over
    (1, ["-gpus", "2", "-gpus_share_device", "1", "-chunk", "40000"], 0, True),          # two contexts (on the one device here): chunks dealt to them in turn
    (1, ["-gpus", "3", "-gpus_share_device", "1", "-gpuparse", "0", "-batch", "200"], 0, True),   # three contexts fed by the host reader
])
def test_real_cli_match_unique(ora, tmp_path, scores, extra, n_list, fastq):
    g = synth.random_genome(80_000, seed=41, n_frag=3, n_runs=6, repeats=15)
    b = synth.concat_batches([synth.sample_reads(g, 1500, 100, 0.02, seed=42, n_read_prob=0.0005),
                              synth.sample_reads(g, 300, 60, 0.02, seed=43)])
    fa, rd = write_inputs(tmp_path, g, b, fastq)
    if "-wrap" in extra:                                           # every sequence line cut in two (FastAReader.hpp:107-138 joins them)
        extra = []
        lines = open(rd).read().split("\n")
        open(rd, "w").write("\n".join(l if l.startswith(">") or not l else l[:37] + "\n" + l[37:] for l in lines))
    out = str(tmp_path / "out.tsv")
    cmd = [REAL, "-t", fa, "-p", rd, "-o", out, "-e", "3", "-s", "2", "-l", "32", "-q", str(scores)] + extra
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    seedl = int(extra[extra.index("-l") + 1]) if "-l" in extra else 32       # (a later -l overrides the one above)
    info, score = oracle_unique(ora, g, b, seedl, 2, 3, scores, n_list, fasta=not fastq)
    want = expected_unique(ora, g, b, info, score, scores)
    got = open(out).read().split("\n")[:-1]
    assert len(got) == len(want)
    assert got == want
    assert ("unique: %d" % len(want)) in r.stderr.decode()


def match_all_case(ora, tmp_path, extra, wrap_record=None):
    """`real -u 0` on the matchAll inputs against the oracle's hit list; wrap_record: sequence and quality of that record
    are cut in two lines each, so that the device parser refuses its chunk and the host reader takes over there"""
    g = synth.random_genome(60_000, seed=51, n_frag=2, repeats=25, repeat_len=200)
    b = synth.sample_reads(g, 800, 100, 0.01, seed=52)
    fa, rd = write_inputs(tmp_path, g, b, True)
    if wrap_record is not None:
        lines = open(rd).read().split("\n")
        assert len(lines) == 4 * 800 + 1
        s, q = lines[4 * wrap_record + 1], lines[4 * wrap_record + 3]
        lines[4 * wrap_record + 1] = s[:41] + "\n" + s[41:]
        lines[4 * wrap_record + 3] = q[:17] + "\n" + q[17:]
        open(rd, "w").write("\n".join(lines))
    out = str(tmp_path / "all.tsv")
    r = subprocess.run([REAL, "-t", fa, "-p", rd, "-o", out, "-u", "0", "-e", "2", "-s", "2", "-l", "32", "-q", "1"] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    err = r.stderr.decode()
    assert ("host reader takes over" in err) == (wrap_record is not None), err[-1500:]
    if wrap_record is not None:                                    # in the middle of the file: not from its first chunk on
        assert 30000 < int(err.split("one-line-per-field form at byte ")[1].split(":")[0]) < os.path.getsize(rd) - 30000
    og = ora.Genome(g.sym, g.frag_start)
    ix = ora.Index(og, 32)
    p = ora.make_params(seedl=32, seedkmax=2, totalkmax=2, scores=1)
    hits, hoff, _ = ora.match_all(og, ix, p, b.bases, b.qual, b.offsets)
    want = []
    for h in hits:
        i = int(h["read"])
        lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
        want.append("\t".join([b.ids[i], seq(b.bases[lo:hi], bool(h["inverted"])), fmt_float(h["score"]), "1", "a", str(hi - lo),
                               "-" if h["inverted"] else "+", g.frag_names[int(h["frag"])],
                               str(int(h["pos"]) - int(g.frag_start[int(h["frag"])]) + 1), "", str(int(h["k"]))]))
    got = open(out).read().split("\n")[:-1]
    assert got == want


@pytest.mark.parametrize("extra", [
    [],
    ["-gpus", "2", "-gpus_share_device", "1", "-batch", "150"],
    ["-gpuparse", "0", "-batch", "150"],                           # read file parsed by the host reader: several blocks
    ["-gpus", "2", "-gpus_share_device", "1", "-gpuparse", "0", "-batch", "150"],   # two contexts fed by the host reader
])
def test_real_cli_match_all(ora, tmp_path, extra):
    match_all_case(ora, tmp_path, extra)


def test_real_cli_match_all_host_reader_takes_over_in_mid_file(ora, tmp_path):
    """record 400 of 800 wrapped and small chunks: the chunks in front of it come from the device parser, the rest of
    the file from the host reader; the lines are those of the regular file"""
    match_all_case(ora, tmp_path, ["-chunk", "30000"], wrap_record=400)


def test_real_cli_errors_are_loud(tmp_path):
    r = subprocess.run([REAL, "-t", "/nonexistent.fa", "-p", "/nonexistent.fq", "-o", str(tmp_path / "o")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode != 0


@pytest.mark.parametrize("irregular", ["wrapped", "blank_line", "crlf"])
def test_real_cli_irregular_record_beyond_the_first_chunk(ora, tmp_path, irregular):
    """A read file that leaves the one-line-per-field form in its middle: the chunks in front of that record are parsed
    on the device, from the refused chunk on the host reader takes over at the right record (small -chunk so that the
    file is many chunks).  "crlf" stays on the device parser all the way; the '\\r' belongs to the id, as in the
    reference (FastQReader.hpp:138-141 reads the id up to the newline)."""
    g = synth.random_genome(80_000, seed=41, n_frag=3, n_runs=6, repeats=15)
    b = synth.sample_reads(g, 1800, 100, 0.02, seed=44, n_read_prob=0.0005)
    fa, rd = write_inputs(tmp_path, g, b, True)
    lines = open(rd).read().split("\n")
    assert len(lines) == 4 * 1800 + 1
    ids = list(b.ids)
    if irregular == "wrapped":                                     # record 900: sequence and quality over two lines each
        s, q = lines[4 * 900 + 1], lines[4 * 900 + 3]
        lines[4 * 900 + 1] = s[:41] + "\n" + s[41:]
        lines[4 * 900 + 3] = q[:17] + "\n" + q[17:]
    elif irregular == "blank_line":
        lines[4 * 1200] = "\n" + lines[4 * 1200]                   # an empty line in front of record 1200
    text = "\n".join(lines)
    if irregular == "crlf":
        text = text.replace("\n", "\r\n")
        ids = [i + "\r" for i in ids]
    open(rd, "w", newline="").write(text)
    out = str(tmp_path / "out.tsv")
    r = subprocess.run([REAL, "-t", fa, "-p", rd, "-o", out, "-e", "3", "-s", "2", "-l", "32", "-q", "1", "-chunk", "30000"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    took_over = "host reader takes over" in r.stderr.decode()
    assert took_over == (irregular != "crlf"), r.stderr.decode()[-1500:]
    info, score = oracle_unique(ora, g, b, 32, 2, 3, 1)
    b2 = synth.ReadBatch(bases=b.bases, qual=b.qual, offsets=b.offsets, ids=ids)
    want = expected_unique(ora, g, b2, info, score, 1)
    got = open(out, newline="").read().split("\n")[:-1]
    assert got == want


def test_real_cli_known_answer_of_the_survey(tmp_path):
    """SURVEY 4 "end-to-end observed": a 36-mer copied from 0-based genome offset 207 and reverse-complemented
    (`p207_inv`) is reported '-', position 208, 0 errors, the printed sequence is the genome substring, and the fragment
    name keeps the space behind '>' (countReads.cpp:46-75)."""
    g = synth.random_genome(1_000_000, seed=1)
    g = synth.Genome(sym=g.sym, frag_start=g.frag_start, frag_names=[" random_1000000"])
    fa = str(tmp_path / "g.fa")
    synth.genome_to_fasta(g, fa)
    assert open(fa).readline() == "> random_1000000\n"
    sub = g.sym[207:243]
    rd = str(tmp_path / "r.fa")
    open(rd, "w").write(">p207_inv\n%s\n" % "".join("ACGT"[c] for c in synth.revcomp(sub)))
    out = str(tmp_path / "o.tsv")
    r = subprocess.run([REAL, "-t", fa, "-p", rd, "-o", out, "-e", "0", "-s", "0", "-l", "32", "-q", "0"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(out).read() == "p207_inv\t%s\t\t1\ta\t36\t-\t random_1000000\t208\t\t0\n" % "".join("ACGT"[c] for c in sub)
    assert "timing: " in r.stderr.decode()


def test_real_cli_long_reads(ora, tmp_path):
    """a read file with 300 and 700 bp reads among 100 bp ones: 300 bp still fit a lane's registers, 700 bp are matched by the wave-per-read kernel"""
    g = synth.random_genome(120_000, seed=45, n_frag=2)
    b = synth.concat_batches([synth.sample_reads(g, 800, 100, 0.02, seed=46), synth.sample_reads(g, 120, 300, 0.005, seed=47),
                              synth.sample_reads(g, 30, 700, 0.002, seed=48)])
    fa, rd = write_inputs(tmp_path, g, b, True)
    out = str(tmp_path / "out.tsv")
    r = subprocess.run([REAL, "-t", fa, "-p", rd, "-o", out, "-e", "3", "-s", "2", "-l", "32", "-q", "1"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    info, score = oracle_unique(ora, g, b, 32, 2, 3, 1)
    want = expected_unique(ora, g, b, info, score, 1)
    got = open(out).read().split("\n")[:-1]
    assert got == want and sum(1 for l in got if l.split("\t")[5] in ("300", "700")) > 60


@pytest.mark.parametrize("extra", [[], ["-block", "25000"], ["-u", "0"]])
def test_real_cli_genome_directory_of_two_files(ora, tmp_path, extra):
    """-t <directory>: every .fa file below it is a genome file with its own file id, in readdir order (getFileList.cpp:145-174;
    matchUniqueImplementation.cpp:1099-1118).  Reads of either file and of a stretch both hold at the same position and
    fragment number: the latter are NonUnique through the file id alone (:131, :219) and must not be printed; the fragment
    name of a printed line is that of ITS file.  Expected lines = the oracle run file by file over the same records, in the
    order `real` says it processed the files."""
    import importlib
    tgp = importlib.import_module("test_gpu_parity")
    g0, g1, b = tgp._two_file_genome()
    d = tmp_path / "genome"
    (d / "sub").mkdir(parents=True)
    synth.genome_to_fasta(g0, str(d / "b_first.fa"))
    synth.genome_to_fasta(g1, str(d / "sub" / "a_second.fa"))
    open(str(d / "notes.txt"), "w").write(">not a genome\nACGT\n")          # (no .fa suffix: ignored)
    rd = str(tmp_path / "reads.fq")
    synth.reads_to_fastq(b, rd)
    out = str(tmp_path / "out.tsv")
    unique = "-u" not in extra
    r = subprocess.run([REAL, "-t", str(d), "-p", rd, "-o", out, "-e", "3" if unique else "2", "-s", "2", "-l", "32", "-q", "1"] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    order = [ln.split("Processing file ")[1].split(" (last")[0].strip() for ln in r.stderr.decode().splitlines() if ln.startswith("Processing file ")]
    assert sorted(os.path.basename(f) for f in order) == ["a_second.fa", "b_first.fa"]
    files = [g0 if os.path.basename(f) == "b_first.fa" else g1 for f in order]
    got = open(out).read().split("\n")[:-1]
    if unique:
        n_list = 25000 if extra else 0
        info = np.zeros(b.n_reads, np.uint64)
        score = np.full(b.n_reads, ora.NOSCORE_INIT, np.float32)
        for fid, g in enumerate(files):
            og = ora.Genome(g.sym, g.frag_start)
            p = ora.make_params(seedl=32, seedkmax=2, totalkmax=3, scores=1, fileid=fid)
            first = 0
            while True:
                ix = ora.Index(og, 32, first, n_list if n_list else 1 << 62)
                info, score, _ = ora.match_unique(og, ix, p, b.bases, b.qual, b.offsets, info=info, score=score)
                first += ix.n
                if not ix.have_next:
                    break
        st, fr, er, fi, po = ora.unpack_record(info)
        want = []
        for i in range(b.n_reads):
            if st[i] not in (1, 2):
                continue
            g = files[fi[i]]
            lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
            want.append("\t".join([b.ids[i], seq(b.bases[lo:hi], st[i] == 2), fmt_float(score[i]), "1", "a", str(hi - lo), "-" if st[i] == 2 else "+",
                                    g.frag_names[fr[i]], str(po[i] - int(g.frag_start[fr[i]]) + 1), "", str(er[i])]))
        assert got == want
        assert sum(1 for l in got if " zero_" in l) > 500 and sum(1 for l in got if " one_" in l) > 400
        assert (st[-200:] == 4).sum() >= 150          # the shared stretch: NonUnique through the file id, not printed (got == want)
    else:
        # matchAll: file by file, block by block, the hits of every read in unifyMatches order (matchAllImplementation.cpp:451-535)
        want = []
        for fid, g in enumerate(files):
            og = ora.Genome(g.sym, g.frag_start)
            p = ora.make_params(seedl=32, seedkmax=2, totalkmax=2, scores=1, fileid=fid)
            hits, hoff, _ = ora.match_all(og, ora.Index(og, 32), p, b.bases, b.qual, b.offsets)
            for h in hits:
                i = int(h["read"])
                lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
                want.append("\t".join([b.ids[i], seq(b.bases[lo:hi], bool(h["inverted"])), fmt_float(h["score"]), "1", "a", str(hi - lo),
                                        "-" if h["inverted"] else "+", g.frag_names[int(h["frag"])],
                                        str(int(h["pos"]) - int(g.frag_start[int(h["frag"])]) + 1), "", str(int(h["k"]))]))
        assert got == want


@pytest.mark.parametrize("fastq", [True, False])
def test_real_cli_patterns_from_stdin(ora, tmp_path, fastq):
    """`real -p -`: the reads piped in give the lines the read file gives (RealOptions.cpp:418-426)."""
    g = synth.random_genome(80_000, seed=41, n_frag=3, n_runs=6, repeats=15)
    b = synth.sample_reads(g, 1200, 100, 0.02, seed=49, n_read_prob=0.0005)
    fa, rd = write_inputs(tmp_path, g, b, fastq)
    out_file, out_pipe = str(tmp_path / "file.tsv"), str(tmp_path / "pipe.tsv")
    base = [REAL, "-t", fa, "-e", "3", "-s", "2", "-l", "32", "-q", "1", "-Q", "33", "-chunk", "50000"]
    r = subprocess.run(base + ["-p", rd, "-o", out_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    env = dict(os.environ, TMPDIR=str(tmp_path))
    r = subprocess.run(base + ["-p", "-", "-o", out_pipe], stdin=open(rd, "rb"), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert "Reading patterns from stdin" in r.stderr.decode() and not list(tmp_path.glob("real_stdin_*"))
    info, score = oracle_unique(ora, g, b, 32, 2, 3, 1, 0, fasta=not fastq)
    want = expected_unique(ora, g, b, info, score, 1)
    assert open(out_pipe).read().split("\n")[:-1] == want == open(out_file).read().split("\n")[:-1]
