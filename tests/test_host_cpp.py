"""CPU tests of the C++ host side (real_amd/host): genome loader, FASTA/FASTQ readers,
host index builder and the RealOptions parser, through the host_selftest binary."""
import os
import subprocess

import numpy as np
import pytest

from real_amd import host_index, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "real_amd", "host", "host_selftest")


@pytest.fixture(scope="module")
def selftest():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "real_amd", "host"), "host_selftest"], stdout=subprocess.DEVNULL)
    return SELFTEST


def test_genome_loader(selftest, tmp_path):
    g = synth.random_genome(5000, seed=3, n_frag=3, n_runs=5)
    fa = tmp_path / "g.fa"
    synth.genome_to_fasta(g, str(fa))
    # quirk 4: anything but ACGTN outside headers is dropped, lowercase included
    txt = open(fa).read().replace("ACG", "ACacgtG", 3).replace("T", "T-", 2)
    open(fa, "w").write(txt)
    subprocess.check_call([selftest, "genome", str(fa), str(tmp_path)])
    sym = np.fromfile(tmp_path / "sym.u8", dtype=np.uint8)
    frag = np.fromfile(tmp_path / "frag.u64", dtype=np.uint64)
    assert np.array_equal(sym, g.sym) and np.array_equal(frag, g.frag_start)
    names = open(tmp_path / "names.txt").read().split("\n")[:-1]
    assert names == g.frag_names                      # header after '>' incl. the leading space
    text, wild = host_index.pack_text(g.sym)
    assert np.array_equal(np.fromfile(tmp_path / "text.u64", dtype=np.uint64), text)
    assert np.array_equal(np.fromfile(tmp_path / "wild.u64", dtype=np.uint64), wild)


@pytest.mark.parametrize("text,sym", [(">a\nAC\n", [0, 1]), (">\nG", [2]), (">x\n", []), ("", [])])
def test_genome_loader_file_shorter_than_the_thread_count(selftest, tmp_path, text, sym):
    """the parallel sweeps cut the file into one piece per thread at line starts; with fewer bytes than threads several
    cuts fall on offset 0, where there is no byte in front to look at (data[-1])"""
    fa = tmp_path / "tiny.fa"
    open(fa, "w").write(text)
    env = dict(os.environ, OMP_NUM_THREADS="64")
    r = subprocess.run([selftest, "genome", str(fa), str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if not sym and r.returncode != 0:
        return                                        # an empty genome may be refused, loudly; it must not crash
    assert r.returncode == 0, r.stderr.decode()
    assert np.fromfile(tmp_path / "sym.u8", dtype=np.uint8).tolist() == sym


def test_fastq_and_fasta_readers(selftest, tmp_path):
    g = synth.random_genome(20000, seed=4)
    b = synth.concat_batches([synth.sample_reads(g, 20, 36, 0.05, seed=5, n_read_prob=0.02),
                              synth.sample_reads(g, 13, 100, 0.05, seed=6)])
    fq = tmp_path / "r.fq"
    synth.reads_to_fastq(b, str(fq), offset=33)
    subprocess.check_call([selftest, "reads", str(fq), "1", "0", str(tmp_path)])
    assert np.array_equal(np.fromfile(tmp_path / "bases.u8", dtype=np.uint8), b.bases)
    assert np.array_equal(np.fromfile(tmp_path / "qual.u8", dtype=np.uint8), b.qual)   # '*'=42 <= 54 -> offset 33 detected
    assert np.array_equal(np.fromfile(tmp_path / "off.u64", dtype=np.uint64), b.offsets)
    assert open(tmp_path / "ids.txt").read().split("\n")[:-1] == b.ids
    assert open(tmp_path / "meta.txt").read().split() == [str(b.n_reads), "33"]
    # Illumina-1.3 style qualities -> 64
    synth.reads_to_fastq(b, str(fq), offset=64)
    subprocess.check_call([selftest, "reads", str(fq), "1", "0", str(tmp_path)])
    assert np.array_equal(np.fromfile(tmp_path / "qual.u8", dtype=np.uint8), b.qual)
    assert open(tmp_path / "meta.txt").read().split()[1] == "64"
    # FASTA: multi-line sequences, lowercase -> 4, constant quality 30
    fa = tmp_path / "r.fa"
    with open(fa, "w") as f:
        for i in range(b.n_reads):
            s = "".join("ACGTN"[c] for c in b.bases[int(b.offsets[i]):int(b.offsets[i + 1])])
            f.write(">" + b.ids[i] + "\n" + s[:10] + "\n" + s[10:] + "\n")
        f.write(">lower\nacgtACGT\n")
    subprocess.check_call([selftest, "reads", str(fa), "0", "0", str(tmp_path)])
    bases = np.fromfile(tmp_path / "bases.u8", dtype=np.uint8)
    assert np.array_equal(bases[:-8], b.bases) and list(bases[-8:]) == [4, 4, 4, 4, 0, 1, 2, 3]
    assert np.all(np.fromfile(tmp_path / "qual.u8", dtype=np.uint8) == 30)
    assert open(tmp_path / "meta.txt").read().split()[0] == str(b.n_reads + 1)


@pytest.mark.parametrize("seedl,threads", [(32, 1), (32, 3), (64, 2), (12, 2)])
def test_host_index_builder(selftest, tmp_path, seedl, threads):
    g = synth.random_genome(30000, seed=7 + seedl, n_frag=2, n_runs=8, repeats=6)
    fa = tmp_path / "g.fa"
    synth.genome_to_fasta(g, str(fa))
    first, mx = 5000, 12000
    subprocess.check_call([selftest, "index", str(fa), str(seedl), str(first), str(mx), str(threads), str(tmp_path)])
    sign, pos, n, nxt = host_index.build_lists(g.sym, seedl, first, mx)
    meta = open(tmp_path / "meta.txt").read().split()
    assert int(meta[0]) == n and bool(int(meta[1])) == nxt and int(meta[2]) == (4 if seedl <= 32 else 8)
    for k in range(6):
        sg = np.fromfile(tmp_path / ("l%d_sign.bin" % k), dtype=np.uint32 if seedl <= 32 else np.uint64)
        ps = np.fromfile(tmp_path / ("l%d_pos.u32" % k), dtype=np.uint32)
        assert np.array_equal(sg, sign[k]) and np.array_equal(ps, pos[k])


def test_realoptions_cpp(selftest, tmp_path):
    fq = tmp_path / "r.fq"
    open(fq, "w").write("@a\nACGT\n+\nIIII\n")
    out = subprocess.check_output([selftest, "options", "-t", "g.fa", "-p", str(fq), "-o", "out", "-e", "30", "-s", "5", "-l", "70",
                                   "-q", "0", "-u", "0", "-filter_level", "3", "--bogus", "-gpus", "2", "-index", "host"],
                                  stderr=subprocess.DEVNULL).decode().split()
    assert out[0] == "g.fa" and out[2] == "out"
    assert out[3:10] == ["2", "15", "64", "0", "0", "0", "3"]
    assert abs(float(out[10]) - 2 * 15 / 70.0) < 1e-6 and out[11:] == ["1", "2", "1"]
    # missing mandatory argument / missing value: error exit, like the reference's exceptions
    assert subprocess.call([selftest, "options", "-t", "g.fa"], stderr=subprocess.DEVNULL) != 0
    assert subprocess.call([selftest, "options", "-t", "g.fa", "-p", str(fq), "-o"], stderr=subprocess.DEVNULL) != 0


def test_realoptions_patterns_from_stdin(selftest, tmp_path):
    """-p - (RealOptions.cpp:418-426, real.cpp:240-257): the patterns come from standard input; they are spooled into a
    temporary file (the driver reads them once per genome block and once more for the output, as the reference does through
    its rewritten pattern file), the format is taken from the first character, and a FASTQ without -Q is taken to be
    Illumina GA (offset 64) with the reference's warning.  The spool file is gone when the options are."""
    env = dict(os.environ, TMPDIR=str(tmp_path))
    r = subprocess.run([selftest, "options", "-t", "g.fa", "-p", "-", "-o", "out"], input=b"@a\nACGT\n+\nhhhh\n", env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    out = r.stdout.decode().split()
    assert out[1].startswith(str(tmp_path)) and "real_stdin_" in out[1] and out[8] == "64" and out[11] == "1"
    assert b"Assuming input" in r.stderr and not os.path.exists(out[1])
    r = subprocess.run([selftest, "options", "-t", "g.fa", "-p", "-", "-o", "out", "-Q", "33"], input=b">a\nACGT\n", env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out = r.stdout.decode().split()
    assert r.returncode == 0 and out[8] == "33" and out[11] == "0" and b"Assuming input" not in r.stderr
    r = subprocess.run([selftest, "options", "-t", "g.fa", "-p", "-", "-o", "out"], input=b"", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode != 0 and not list(tmp_path.glob("real_stdin_*"))       # empty input: the reference's error, and no file left behind


def test_fast_score_formatter_equals_printf(selftest):
    """the score column: fastformat::fmt_g6 (integer arithmetic) against printf's %g -- which is what the reference's
    operator<<(float) prints -- on random bit patterns, score-like values, integers and both sides of every power of ten"""
    r = subprocess.run([selftest, "fmtcheck", "400000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "0", r.stderr[-2000:]


@pytest.mark.parametrize("threads,crlf", [(1, False), (7, False), (7, True)])
def test_output_lines_from_blocks_and_from_text(selftest, tmp_path, threads, crlf):
    """the 11-column lines (real_amd/host/Lines.hpp) of every read of a file, formatted from the host reader's blocks and
    from the file as one text chunk: both equal the lines built here with the formula of expected_unique
    (tests/test_cli_gpu.py).  Placement of read r, as `host_selftest lines` states it: '-' for odd r, no score for
    r % 3 == 2, positions up to 2^35 - 1, errors r % 16, one name with a leading space.  Anything but ACGT prints as N;
    7 threads on blocks of 7 reads and a read of one base: empty thread ranges; CRLF: the '\\r' belongs to the id."""
    g = synth.random_genome(20000, seed=4)
    b = synth.concat_batches([synth.sample_reads(g, 20, 36, 0.05, seed=5, n_read_prob=0.05),
                              synth.sample_reads(g, 1, 1, 0.0, seed=7),
                              synth.sample_reads(g, 19, 100, 0.05, seed=6, n_read_prob=0.01)])
    assert (b.bases == 4).any()
    fq = tmp_path / "r.fq"
    names = [" chr one", "two", " 3"]
    nl = "\r\n" if crlf else "\n"
    want = []
    with open(fq, "w", newline="") as f:
        for r in range(b.n_reads):
            lo, hi = int(b.offsets[r]), int(b.offsets[r + 1])
            bases = b.bases[lo:hi].copy()
            text = ["ACGTN"[c] for c in bases]
            for k in range(r % 5, hi - lo, 11):                   # lowercase letters: not ACGT, so N
                text[k] = text[k].lower()
                bases[k] = 4
            f.write("@" + b.ids[r] + nl + "".join(text) + nl + "+" + nl + "I" * (hi - lo) + nl)
            inv = r % 2 == 1
            pos1 = ((r * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) >> 29
            pos1 = {0: 2 ** 35 - 1, 1: 1}.get(r, pos1)
            score = "%g" % float(np.float32((r * 7919 % 100003 - 50000) / 16.0))
            seq = "".join("ACGTN"[c] for c in (synth.revcomp(bases) if inv else bases))
            want.append("\t".join([b.ids[r] + ("\r" if crlf else ""), seq, score if r % 3 != 2 else "", "1", "a", str(hi - lo), "-" if inv else "+",
                                   names[r % 3], str(pos1), "", str(r % 16)]))
    subprocess.check_call([selftest, "lines", str(fq), str(tmp_path)], env=dict(os.environ, OMP_NUM_THREADS=str(threads)))
    assert len(want) == 40 and max(len(w) for w in want) > 150
    for name in ("block.tsv", "chunk.tsv"):
        assert open(tmp_path / name, newline="").read().split("\n")[:-1] == want, name


def test_final_record_decoders(selftest):
    """csrc/final_record.h, the one decoder of info words, pair records and single records that the stages behind the matcher
    share, compiled by the host compiler: `host_selftest records` checks it against records written through the public
    structs and macros of real_hip.h -- every state, both strands, both mates, the file ids and positions at the ends of
    their ranges -- and against info words as Lines.hpp's unpack reads them (35-bit positions included)."""
    r = subprocess.run([selftest, "records"], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout


def test_table_plan(selftest):
    """csrc/index_plan.h's rh_plan_tables -- which layout and prefix width an index gets -- compiled by the host compiler:
    `host_selftest plan` prints it over seedl x request x prefix_bits x entries x device memory x no_rows (15120 lines,
    the large-index branches included, which no GPU test reaches).  The whole output is pinned to what the function
    printed when it still sat in index_build.hip; the rows spelled out are there for the reader.
    Layouts: 0 bucket starts, 1 digest directory, 2 fingerprint directory, 3 bucket rows."""
    import hashlib
    r = subprocess.run([selftest, "plan"], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 10 * 4 * 7 * 9 * 3 * 2
    G16, G288, HUGE = 16 << 30, 288 << 30, 1 << 62
    want = {
        # l request prefix_bits n_entries device_bytes no_rows -> pb layout
        (32, 0, 0, 3_000_000_000, G288, 0): (28, 3),   # BASELINE: a 3 Gbp genome on 288 GiB gets bucket rows, 2^28 of them
        (32, 0, 0, 3_000_000_000, G288, 1): (29, 1),   # ... the rows did not fit once: digest directories, all bits but three
        (32, 0, 0, 3_000_000_000, G16, 0): (29, 1),    # ... a 16 GiB device: no room for the rows
        (64, 0, 0, 3_000_000_000, G288, 0): (28, 3),   # 64-bit signatures: rows too
        (64, 0, 0, 3_000_000_000, G16, 0): (29, 2),    # ... and fingerprint directories where they do not fit
        (32, 0, 0, (1 << 27) - 1, G288, 0): (25, 0),   # one entry below `big`: bucket starts, mean bucket 2..4
        (32, 0, 0, 1 << 27, G288, 0): (29, 1),         # big, but 2^28 rows would hold half an entry each: digest directories
        (32, 1, 0, 3_000_000_000, G288, 0): (30, 0),   # bucket starts on request: the prefix stops at 30 bits
        (12, 0, 0, 1000, G16, 0): (8, 0),              # a tiny index: at least 8 prefix bits
        (16, 3, 12, 32000, G16, 0): (12, 3),           # rows on request, four group bits
        (16, 2, 13, 32000, G16, 0): (13, 1),           # a directory on request, three bits below the prefix: digest
        (64, 2, 13, 32000, G16, 0): (13, 2),          # ... wide signatures: fingerprints
        (48, 0, 0, (1 << 32) - 1, HUGE, 0): (29, 0),   # seedl 48: no 32 key bits below a row prefix, and an entry holds all 19 bits below this one: bucket starts
    }
    got = {}
    for line in lines:
        a, b = line.split(" -> ")
        got[tuple(int(x) for x in a.split())] = tuple(int(x) for x in b.split())
    assert len(got) == len(lines)
    assert {k: got[k] for k in want} == want
    assert hashlib.sha256(r.stdout.encode()).hexdigest() == "ba72e8f549613b49c08bd4ce9a3fac91d500e77d89c5a924c8cf4a492297364d"


def test_gap_record_geometry_against_the_checkers_rule(selftest):
    """csrc/final_record.h's rh_gap_fit, the one geometry rule of the stages that consume gap records, against the rule of
    tests/gapped_list_checker.py over `host_selftest gap_grid`: L in {1, 2, 31, 32, 33, 320, 321}, g in -17 .. 17, every split
    0 .. L + 1, spans that end one before, on and one behind the text's end, and the position 0xFFFFFF00.  (`host_selftest
    records` above checks the decoder of the record's fields.)"""
    import gapped_list_checker as glc
    n = 100_013
    r = subprocess.run([selftest, "gap_grid", str(n)], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0
    got = np.array([line.split() for line in r.stdout.split("\n")[:-1]], dtype=np.int64)
    assert got.shape == (sum(L + 2 for L in (1, 2, 31, 32, 33, 320, 321)) * 35 * 4, 7)
    assert set(got[:, 0]) == {1, 2, 31, 32, 33, 320, 321} and set(got[:, 1]) == set(range(-17, 18)) and (got[:, 3] == 0xFFFFFF00).sum() * 4 == got.shape[0]
    bad = [row.tolist() for row in got
           if (bool(row[4]), row[5], row[6]) != (glc.fits({"gap": row[1], "split": row[2], "pos": row[3]}, int(row[0]), n), max(-row[1], 0), max(row[1], 0))]
    assert not bad, bad[:10]
    fit = got[got[:, 4] == 1]
    assert 0 < fit.shape[0] < got.shape[0] // 3 and set(fit[:, 0]) == {1, 2, 31, 32, 33, 320}      # (L = 1 fits without a gap only)
    assert not fit[fit[:, 0] == 1][:, 1].any() and set(fit[:, 1]) == set(range(-16, 17)) and (fit[:, 3] + fit[:, 0] + fit[:, 1] <= n).all()


def _chunk_records(fmt, nl, final_newline):
    """seven records of lengths 1, 36, 100, 1, 5, 100, 2 with ids of different lengths, one line per field"""
    recs = []
    for k, n in enumerate([1, 36, 100, 1, 5, 100, 2]):
        rid, seq = "r" + "x" * (3 * k) + str(k), "ACGT" * (n // 4) + "ACGT"[:n % 4]
        recs.append(("@" + rid + nl + seq + nl + "+" + nl + "I" * n + nl) if fmt == "fastq" else (">" + rid + nl + seq + nl))
    if not final_newline:
        recs[-1] = recs[-1][:-len(nl)]
    return [r.encode() for r in recs]


@pytest.mark.parametrize("buffers", [1, 2])
@pytest.mark.parametrize("fmt,nl,final_newline", [("fastq", "\n", True), ("fasta", "\n", True), ("fastq", "\r\n", True), ("fastq", "\n", False),
                                                  ("empty", "\n", True)])
def test_read_chunks(selftest, tmp_path, fmt, nl, final_newline, buffers):
    """RawChunker (real_amd/host/RawChunker.hpp) through `host_selftest chunks`: the text chunks of a read file, with malloc'd
    buffers.  What must hold follows from the file alone: the chunks concatenated are the file, file_offset is the running sum
    of the sizes, no chunk is empty or larger than the capacity, and every chunk but the last ends behind a newline and holds a
    multiple of 4 (FASTQ) or 2 (FASTA) lines -- whole records.  Capacities: exactly the longest record, one byte more, the
    longest plus the shortest, the whole file, the whole file plus one; one buffer (every chunk is handed back before the next
    is read) and two (the prefetch runs ahead).  An empty file gives no chunk.  A capacity below the longest record ends with
    the message of `real` and a non-zero status."""
    recs = [] if fmt == "empty" else _chunk_records(fmt, nl, final_newline)
    data = b"".join(recs)
    path, out = tmp_path / "reads.txt", tmp_path / "chunks.bin"
    open(path, "wb").write(data)
    fastq, lpr = ("0", 2) if fmt == "fasta" else ("1", 4)

    def run(cap):
        r = subprocess.run([selftest, "chunks", str(path), fastq, str(cap), str(buffers), str(out)], stderr=subprocess.PIPE, universal_newlines=True)
        raw, chunks, at = open(out, "rb").read(), [], 0
        while r.returncode == 0 and at < len(raw):
            off, size = (int(v) for v in np.frombuffer(raw[at:at + 16], dtype=np.uint64))
            chunks.append((off, raw[at + 16:at + 16 + size]))
            assert len(chunks[-1][1]) == size
            at += 16 + size
        return r, chunks

    if not recs:
        r, chunks = run(64)
        assert r.returncode == 0 and chunks == []
        return
    longest, shortest = max(len(r) for r in recs), min(len(r) for r in recs)
    for cap in (longest, longest + 1, longest + shortest, len(data), len(data) + 1):
        r, chunks = run(cap)
        assert r.returncode == 0, (cap, r.stderr)
        assert b"".join(c for _, c in chunks) == data, cap
        assert [off for off, _ in chunks] == [int(v) for v in np.cumsum([0] + [len(c) for _, c in chunks[:-1]])], cap
        assert all(0 < len(c) <= cap for _, c in chunks), cap
        assert all(c.endswith(b"\n") and c.count(b"\n") % lpr == 0 for _, c in chunks[:-1]), cap
        assert len(chunks) > 1 or cap >= len(data), cap
    r, chunks = run(longest - 1)
    assert r.returncode != 0 and r.returncode > 0 and "a read record longer than the text chunk" in r.stderr, (r.returncode, r.stderr)
