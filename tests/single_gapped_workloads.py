"""The single-end workload of the gapped consumers -- TEST INFRASTRUCTURE ONLY.  A function of its seed: the mates
of indel_workloads.planted() as single reads (mate 1's batch, then mate 2's, with their qualities), behind them PCR copies -- every
10th read once more with new qualities, and every 15th read from 5 on cut to its first 60 bases (the same 5' end with a shorter
span: the cut copy of a read that carries an indel behind base 60 is placed UNGAPPED, and meets its gapped original in one group).
oracle_*: the oracle's final info words and the checker's gap records, read summaries and joint marks of a run."""
from __future__ import annotations

import functools
import types

import numpy as np

import dup_checker as dk
import dup_gapped_checker as dgk
import gap_anchor_checker as gac
import gap_checker as gc
import indel_workloads as iw

SEEDL, SEEDKMAX, TOTALKMAX = 32, 1, 1
FLAGS = ["-e", str(TOTALKMAX), "-s", str(SEEDKMAX), "-l", str(SEEDL), "-q", "0", "-filter_level", "0", "-Q", "33"]
AP = gac.AnchorParams(32, 32)                    # -gap_anchor / -gap_anchors of the run (the defaults for -l 32)
CUT = 60
MIN_QUAL = 15                                    # -dedup_minq's default


@functools.lru_cache(maxsize=None)
def workload(seed=7):
    """-> namespace: g, b (the single reads, ids r0 ..), n_base (the reads that are no copies), copy_of [(copy, original)], plants,
    prm (the gap parameters), planted (indel_workloads' namespace)"""
    p = iw.planted(seed)
    reads, quals = [], []
    for b in (p.b1, p.b2):
        for i in range(b.n_reads):
            lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
            reads.append(b.bases[lo:hi].copy())
            quals.append(b.qual[lo:hi].copy())
    n_base = len(reads)
    rng = np.random.default_rng(3)
    copy_of = []
    for i in range(0, n_base, 10):
        copy_of.append((len(reads), i))
        reads.append(reads[i].copy())
        quals.append(rng.integers(25, 41, size=reads[i].shape[0]).astype(np.uint8))
    for i in range(5, n_base, 15):
        copy_of.append((len(reads), i))
        reads.append(reads[i][:CUT].copy())
        quals.append(quals[i][:CUT].copy())
    b = iw.Batch(reads, quals, ["r%d" % i for i in range(len(reads))])
    return types.SimpleNamespace(g=p.g, b=b, n_base=n_base, copy_of=copy_of, plants=p.plants, prm=gc.default_params(TOTALKMAX), planted=p, fileid=0)


@functools.lru_cache(maxsize=None)
def second_genome(seed=7):
    """the other genome file of the two-file variant, and reads of its own: some exact, some with one deleted base"""
    from real_amd import synth
    g = synth.random_genome(20_000, seed + 101, n_frag=2, n_runs=0)
    rng = np.random.default_rng(seed + 102)
    fs = [int(v) for v in g.frag_start]
    reads, quals = [], []
    for k in range(120):
        f = k & 1
        s = int(rng.integers(fs[f] + 10, fs[f + 1] - 130))
        r = g.sym[s:s + 101].copy()
        r = np.delete(r, 50)[:100] if k % 3 == 0 else r[:100]        # (every third one: a read with one base missing, a deletion)
        if k % 3 == 1 and k % 2:
            r = np.concatenate([r[:40], [(r[40] + 1) & 3, (r[41] + 2) & 3], r[40:98]]).astype(np.uint8)     # two inserted bases
        if k & 2:
            r = gc.COMP[r[::-1]]
        reads.append(r.astype(np.uint8))
        quals.append(rng.integers(25, 41, size=100).astype(np.uint8))
        if k % 4 == 0:                                                # a copy of it, of lower quality
            reads.append(reads[-1].copy())
            quals.append((quals[-1] - 5).astype(np.uint8))
    return g, reads, quals


@functools.lru_cache(maxsize=None)
def two_files(seed=7):
    """the two-file variant: the workload's genome as file 0 and a second random genome as file 1, the workload's first 1500 reads
    (and their share of the copies is gone: the reads are fewer, the run quicker) with reads of the second genome behind them"""
    w = workload(seed)
    g2, r2, q2 = second_genome(seed)
    n0 = 1500
    reads = [w.b.read(i).copy() for i in range(n0)] + r2
    quals = [w.b.qual[int(w.b.offsets[i]):int(w.b.offsets[i + 1])].copy() for i in range(n0)] + q2
    b = iw.Batch(reads, quals, ["r%d" % i for i in range(len(reads))])
    return types.SimpleNamespace(g=w.g, g2=g2, b=b, prm=w.prm, fileid=0)


def oracle_run(ora, b, genomes, prm, per_block=1 << 62):
    """(info, gaps, n_blocks) of a run over the genome files `genomes` (file ids in their order), index blocks of per_block
    entries: the oracle's final info words; the gap records of gap_anchor_checker over every block, folded"""
    sub = gac.SubBatch(b, AP.anchor_len)
    info, blocks = None, []
    for fid, g in enumerate(genomes):           # (gap_anchor_workloads.oracle_run with this run's -s)
        og = ora.Genome(g.sym, g.frag_start)
        p = ora.make_params(seedl=SEEDL, seedkmax=SEEDKMAX, totalkmax=TOTALKMAX, scores=False, filter_level=0, fileid=fid)
        first = 0
        while True:
            ix = ora.Index(og, SEEDL, first, per_block)
            info, _, _ = ora.match_unique(og, ix, p, b.bases, b.qual, b.offsets, info=info)
            hits, hoff, _ = ora.match_all(og, ix, p, sub.bases, sub.qual, sub.offsets)
            blocks.append((fid, g, hits, hoff))
            first += ix.n
            if not ix.have_next:
                break
    rec = None
    for fid, g, hits, hoff in blocks:           # (the gapped pass runs behind the matching: every block sees the FINAL info words)
        rec, _ = gac.check_anchor(gc.Text(g.sym, g.frag_start, fid), b, info, hits, hoff, prm, AP, out=rec)
    return info, rec, len(blocks)


_cache = {}


def expected(ora, seed=7):
    """(info, gaps, sums, dup, stats, groups) of the one-file workload: the oracle's records and the checkers' marks, computed once"""
    if seed not in _cache:
        w = workload(seed)
        info, gaps, _ = oracle_run(ora, w.b, [w.g], w.prm)
        sums = dk.summaries_of(w.b, MIN_QUAL)
        _cache[seed] = (info, gaps, sums) + dgk.mark_groups(info, gaps, sums)
    return _cache[seed]


# ---- hand-made arrays for the marking alone (it needs neither text nor index) ----------------------------------------------------
HAND_N = (0, 1, 63, 64, 65, 255, 256, 257, 4099)     # around the wave and the block of 256, and more than a few blocks
HAND_GAPS = (-16, -1, 0, 1, 16)
HAND_LENGTHS = (1, 25, 100, 320, 16384)
HAND_FILES = (0, 1, 63)
Q_TOP = (1 << 20) - 1


def info_word(state, pos, fileid=0):
    return (state << 61) | (fileid << 35) | pos


def hand(n, seed=1):
    """(info, gaps, sums) of n reads: every state of both records (info 0..4, gap 0..3), both strands, every gap of HAND_GAPS and
    length of HAND_LENGTHS, the file ids 0 / 1 / 63, 5' ends drawn from a pool of eight per file and strand -- so that the kinds
    meet in groups --, the qualities from a few values with qsum at and beyond 2^20 - 1 among them (ties: the smallest index
    stays).  The position of a read follows from its 5' end: END5 - len + 1 (reverse info word), END5 - len - gap + 1 (reverse
    gap record)"""
    rng = np.random.default_rng(seed * 1000 + n)
    info = np.zeros(n, dtype=np.uint64)
    gaps = gc.empty_records(n)
    sums = np.zeros(n, dtype=dk.SUM_DTYPE)
    pool = 40_000 + 37 * np.arange(8)            # (beyond the longest read and the widest gap: no position below 0)
    for i in range(n):
        ist, gst = int(rng.integers(0, 5)), int(rng.integers(0, 4))
        if i % 3 == 0:
            ist = 0                               # (a third of the reads surely left to their gap record)
        L = HAND_LENGTHS[int(rng.integers(0, len(HAND_LENGTHS)))]
        g = HAND_GAPS[int(rng.integers(0, len(HAND_GAPS)))]
        fid = HAND_FILES[int(rng.integers(0, 3))]
        e5 = int(pool[int(rng.integers(0, 8))])
        e5g = int(pool[int(rng.integers(0, 8))])
        inv = int(rng.integers(0, 2))
        sums[i] = (L, (700, 700, 900, Q_TOP - 1, Q_TOP, Q_TOP + 1, 1 << 21)[int(rng.integers(0, 7))])
        info[i] = info_word(ist, e5 - L + 1 if ist == 2 else e5, fid)
        gaps[i]["pos"] = e5g - L - g + 1 if inv else e5g
        gaps[i]["fileid"], gaps[i]["gap"], gaps[i]["tag"] = fid, g, dgk.gap_tag(gst, inv)
        gaps[i]["split"], gaps[i]["k"], gaps[i]["cost"] = (1 if g else 0), int(rng.integers(0, 4)), int(rng.integers(0, 30))
    return info, gaps, sums


def hand_edges():
    """(info, gaps, sums, dup) by hand.  0-2: a reverse gap record at pos 0xFFFFFF00 -- its END5 = 0xFFFFFF00 + 320 + 16 - 1 lies
    beyond 2^32 -- with a reverse info word of ten bases that ends there (bit 32 of its position set) and a better copy of the record;
    3-4: reverse gap records of one base with 16 inserted: END5 = 3 + 1 - 16 - 1 < 0 is 2^36 - 13, where the two meet;
    5-6: an info word wins over its Unique gap record (the record's key is 0's group, the word's another one);
    7-8: a NonUnique and a NoMatch gap record at 0's key place nothing; 9: file id 63, the same END5: a group of its own;
    10-11: equal qsum, the smaller index stays; 12-13: qsum 2^20 - 1 and 2^20 + 7 are equal"""
    top = 0xFFFFFF00
    e5 = top + 320 + 16 - 1
    assert e5 > 1 << 32 and e5 - 10 + 1 > 1 << 32
    rows = [  # (info state, info pos, gap state, inv, gap pos, gap, len, qsum, fileid)
        (0, 0, 1, 1, top, 16, 320, 500, 0), (2, e5 - 10 + 1, 0, 0, 0, 0, 10, 400, 0), (0, 0, 1, 1, top, 16, 320, 600, 0),
        (0, 0, 1, 1, 3, -16, 1, 30, 0), (4, 9, 1, 1, 3, -16, 1, 40, 0),
        (1, 77, 1, 1, top, 16, 320, 900, 0), (1, 77, 0, 0, 0, 0, 320, 100, 0),
        (0, 0, 2, 1, top, 16, 320, 9000, 0), (3, 0, 0, 1, top, 16, 320, 9000, 0), (0, 0, 1, 1, top, 16, 320, 100, 63),
        (0, 0, 1, 0, 5000, 3, 100, 800, 1), (1, 5000, 0, 0, 0, 0, 60, 800, 1),
        (2, 6000 - 99, 0, 0, 0, 0, 100, Q_TOP, 1), (0, 0, 1, 1, 6000 - 100 - (-2) + 1, -2, 100, Q_TOP + 7, 1)]
    n = len(rows)
    info = np.zeros(n, dtype=np.uint64)
    gaps = gc.empty_records(n)
    sums = np.zeros(n, dtype=dk.SUM_DTYPE)
    for i, (ist, ipos, gst, inv, gpos, g, L, q, fid) in enumerate(rows):
        info[i] = info_word(ist, ipos, fid)
        gaps[i]["pos"], gaps[i]["gap"], gaps[i]["fileid"], gaps[i]["tag"], gaps[i]["split"] = gpos, g, fid, dgk.gap_tag(gst, inv), 1 if g else 0
        sums[i] = (L, q)
    dup = np.array([1, 1, 0,  1, 0,  0, 1,  0, 0, 0,  0, 1,  0, 1], dtype=np.uint8)
    return info, gaps, sums, dup
