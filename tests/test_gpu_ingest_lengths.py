"""real_hip_parse_reads at the lengths where its kernels change form -- one lane per record up to 128 bases, 64 lanes per
record beyond, more than one 256-base chunk from 257 on -- up to the longest read of the library, with quality characters up
to '~' for both offsets, text at a 16-byte aligned, a 4-byte aligned and an odd device address, LF and CRLF line ends; and a
record without bases.  Compared with the generator's arrays and, for the empty record, with the host reader."""
import os
import subprocess

import numpy as np
import pytest

from real_amd import lib as rlib
from real_amd.matcher import RealOptions, UniqueMatcher

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "real_amd", "host", "host_selftest")
BASES = np.frombuffer(b"ACGTN", dtype=np.uint8)
LENGTHS = (1, 128, 129, 256, 257, 2048, 16384)


class _Batch:
    pass


def _fastq(b, qoff=33, crlf=False, trailing_newline=True):
    """(the helper of test_gpu_ingest.py)"""
    nl = b"\r\n" if crlf else b"\n"
    parts = []
    for i in range(len(b.offsets) - 1):
        lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
        parts += [b"@" + b.ids[i].encode(), BASES[b.bases[lo:hi]].tobytes(), b"+", (b.qual[lo:hi] + qoff).astype(np.uint8).tobytes()]
    return nl.join(parts) + (nl if trailing_newline else b"")


_B = {}


def _reads(qoff, with_empty=False):
    """100-base reads with two reads of every length of LENGTHS among them, some bases N; qualities up to '~' - qoff, the
    largest one first and last in every read of 2 bases and more"""
    key = (qoff, with_empty)
    if key not in _B:
        rng = np.random.default_rng(100 + qoff)
        top = ord("~") - qoff
        lens = [100] * 40 + list(LENGTHS) * 2 + ([0, 0] if with_empty else [])
        lens = [lens[i] for i in rng.permutation(len(lens))]
        if with_empty:                                          # (also: the first and the last record)
            lens = [0] + lens + [0]
        b = _Batch()
        b.bases = np.concatenate([rng.choice(5, size=L, p=[0.245, 0.245, 0.245, 0.245, 0.02]) for L in lens] + [np.zeros(0, np.int64)]).astype(np.uint8)
        b.qual = rng.integers(0, top + 1, size=b.bases.shape[0]).astype(np.uint8)
        b.offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        for i, L in enumerate(lens):
            if L >= 2:
                b.qual[int(b.offsets[i])] = b.qual[int(b.offsets[i + 1]) - 1] = top
        b.ids = ["r%d_L%d" % (i, L) for i, L in enumerate(lens)]
        _B[key] = b
    return _B[key]


def _check(m, p, b, text):
    n = len(b.offsets) - 1
    assert p.n_reads == n and p.n_symbols == int(b.offsets[-1])
    assert np.array_equal(m.download(p.offsets, n + 1, np.uint64), b.offsets)
    bases, qual = m.download(p.bases, int(p.n_symbols), np.uint8), m.download(p.qual, int(p.n_symbols), np.uint8)
    assert np.array_equal(bases, b.bases), np.nonzero(bases != b.bases)[0][:10]
    assert np.array_equal(qual, b.qual), np.nonzero(qual != b.qual)[0][:10]
    assert p.max_patl == int(np.diff(b.offsets.astype(np.int64)).max()) == rlib.REAL_HIP_MAX_PATL_LONG
    ids0, idl = m.download(p.id_start, n, np.uint32), m.download(p.id_len, n, np.uint32)
    assert [text[int(s):int(s) + int(l)].decode() for s, l in zip(ids0, idl)] == b.ids


def _placed(text, where):
    """the text as host bytes or at a device address that is 16-byte aligned, 4-byte aligned or odd"""
    if where == "host":
        return text
    import torch
    shift = {"16": 0, "4": 4, "odd": 1}[where]
    t = torch.frombuffer(bytearray(b"#" * shift + text), dtype=torch.uint8).cuda()
    assert t.data_ptr() % 16 == 0
    return t[shift:]


@pytest.mark.parametrize("where", ["host", "16", "4", "odd"])
@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("qoff", [33, 64])
def test_every_length_and_quality_character(qoff, crlf, where):
    b = _reads(qoff)
    assert int(b.qual.max()) == ord("~") - qoff and (qoff == 64 or int(b.qual.max()) == 93) and (b.bases == 4).any()
    text = _fastq(b, qoff, crlf)
    m = UniqueMatcher(RealOptions(seedl=32, seedkmax=2, totalkmax=3, scores=True).normalise())
    _check(m, m.parse_reads(_placed(text, where), fastq=True, quality_offset=qoff), b, text)
    if where == "odd" and not crlf:
        _check(m, m.parse_reads(_placed(text[:-1], where), fastq=True, quality_offset=qoff), b, text)      # (no final newline)
    m.close()


@pytest.mark.parametrize("where", ["host", "odd"])
@pytest.mark.parametrize("crlf", [False, True])
def test_a_record_without_bases_is_what_the_host_reader_makes_of_it(tmp_path, crlf, where):
    """an empty sequence line and an empty quality line: the host ReadReader gives a read of length 0, and so does the device
    parser (first record, last record and two in the middle)"""
    b = _reads(33, with_empty=True)
    lens = np.diff(b.offsets.astype(np.int64))
    assert lens[0] == 0 and lens[-1] == 0 and (lens == 0).sum() == 4
    text = _fastq(b, 33, crlf)
    fq = tmp_path / "e.fq"
    fq.write_bytes(text)
    subprocess.check_call([SELFTEST, "reads", str(fq), "1", "33", str(tmp_path)])
    assert np.array_equal(np.fromfile(tmp_path / "off.u64", dtype=np.uint64), b.offsets)
    assert np.array_equal(np.fromfile(tmp_path / "bases.u8", dtype=np.uint8), b.bases)
    assert np.array_equal(np.fromfile(tmp_path / "qual.u8", dtype=np.uint8), b.qual)
    m = UniqueMatcher(RealOptions(seedl=32, seedkmax=2, totalkmax=3, scores=True).normalise())
    _check(m, m.parse_reads(_placed(text, where), fastq=True, quality_offset=33), b, text)
    m.close()


def test_records_without_bases_only():
    """three records, no base: the parsed arrays are a batch the matcher takes (every read NoMatch)"""
    m = UniqueMatcher(RealOptions(seedl=32, seedkmax=2, totalkmax=3, scores=True).normalise())
    m.set_text_symbols(0, np.random.default_rng(1).integers(0, 4, size=5000).astype(np.uint8), np.array([0, 5000], dtype=np.uint64))
    m.build_index_block()
    p = m.parse_reads(b"@a\n\n+\n\n@b\n\n+\n\n@c\n\n+\n\n", fastq=True, quality_offset=33)
    assert p.n_reads == 3 and p.n_symbols == 0 and p.max_patl == 0
    assert not m.download(p.offsets, 4, np.uint64).any()
    info, score = m.match_unique_parsed(p)
    assert info.shape[0] == 3 and not info.any()
    m.close()
