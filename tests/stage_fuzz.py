"""Randomised chains of the placement stages -- TEST INFRASTRUCTURE ONLY ("stage fuzz").

draw(kind, seed)      a configuration: a frozen dataclass of plain values, a function of (kind, seed) alone
workload(cfg)         the reads and the genome files of a configuration: gap_workloads / gap_anchor_workloads with the drawn
                      arguments, PCR copies (and, single-end, cut copies as single_gapped_workloads makes them) behind them
expected(cfg, ora)    every stage's expected output, from the oracle's hit lists through the existing checkers, each stage fed
                      the previous stage's expected output; cached per (kind, seed)
run(cfg, ora, make)   the same chain on the device through real_amd.matcher, one context per configuration; after every stage
                      the outputs are compared with expected() before the next stage runs
check_stage           the comparison path alone (no device): every output of a stage through the checkers' assert helpers; a
                      difference raises StageDiff with the stage's name and repr(cfg)

A stage runs once on the whole batch and once as two calls on [0, c) and [c, n): records concatenate to the whole, accumulating
stages sum to it.  The batch is presented to every stage of a configuration in one drawn way (host arrays, device arrays,
device reads with host records, packed bases whose first read starts inside a byte).  Nothing is skipped and no exception is
caught and passed over: a configuration the library refuses is a bug of draw().
"""
from __future__ import annotations

import dataclasses
import hashlib
import types
from typing import Optional, Tuple

import numpy as np

import dup_checker as dk
import dup_gapped_checker as dgk
import gap_anchor_checker as gac
import gap_anchor_workloads as aw
import gap_checker as gc
import gap_workloads as gw
import gapped_list_checker as glc
import indel_checker as ic
import insert_checker as ik
import mapq_checker as mq
import mate_search_checker as mc
import pairs_all_checker as pac
import pairs_checker as pc
import pileup_gapped_checker as pgc
import sam_checker as sk
import single_gapped_workloads as sgw
import singles_checker as sc

KINDS = {"paired": 0, "single": 1}
MATE_SEARCH_MAX_INSERT = 4096          # REAL_HIP_MATE_SEARCH_MAX_INSERT

# ---- the domain (DESIGN.md holds the table) ---------------------------------------------------------------------------------
SEEDLS = (16, 20, 24, 32, 48, 64)
TABLE_KINDS = (0, 0, 2, 3, 3)          # fuzz_parity.py's draw: auto (bucket starts), directory entries, bucket rows
FILTER_LEVELS = (0, 1, 2, 3)
FILE_IDS = (0, 1, 5, 63)
MARGINS = (0, 1, 3)
PILEUP_MINQ = (0, 13, 20, 30)
MIN_CALL_QUAL = (0, 10, 20)
MIN_DEPTH = (1, 2, 4)
MIN_ALT = (1, 2, 3)
DEDUP_MINQ = (0, 15, 30)
HIST_BINS = (64, 1024, 16384)
PRESENTATIONS = ("host", "device", "mixed", "packed")
TARGET_LENGTHS = (25, 31, 32, 33, 47, 64, 65, 96, 100, 127, 150, 200, 255, 256, 257, 320)
ANCHOR_MATE_LENGTHS = (64, 100, 150)
WINDOWS = (1, 63, 64, 65)              # concordant starts: the tile of 64 lanes and its neighbours
SEARCH_ANCHORS = (0, 4)
SINGLE_ANCHORS = (1, 4, 32, 64)
CUTS = ("zero", "all", "inside")
LAYOUTS = ("starts", "digest", "fingerprint", "rows", "wide rows")


@dataclasses.dataclass(frozen=True)
class Config:
    kind: str
    seed: int
    # matcher
    seedl: int
    table_kind: int
    prefix_bits: int
    seedkmax: int
    totalkmax: int
    scores: int
    filter_level: int
    # qualities: None = independent per base in 0..63 with runs of 0, else the constant
    qual_const: Optional[int]
    # genome
    size: int
    n_frag: int
    n_runs: int
    fileids: Tuple[int, ...]
    # gap parameters
    max_gap: int
    min_flank: int
    margin: int
    max_cost: Optional[int]
    # consumers
    pileup_minq: int
    min_call_qual: int
    min_depth: int
    min_alt: int
    dedup_minq: int
    dedup: int
    hist_bins: int
    # how the batch is handed over
    presentation: str
    garbage_out: int
    cut: str
    cut_frac: float
    gapped_first: int
    second_half_first: int
    # reads
    patl: int
    n: int
    # paired only
    anchor_l: int = 0
    frag_l: int = 0
    min_ins: int = 0
    max_ins: int = 0
    mate_search: int = 0
    search_anchors: int = 0
    # single only
    anchor_len: int = 0
    max_anchors: int = 0
    n_blocks: int = 0

    @property
    def layout(self) -> str:
        """the index layout the drawn table kind asks for at this seed length"""
        if self.table_kind == 0:
            return "starts"
        if self.table_kind == 2:
            return "digest" if self.seedl <= 32 else "fingerprint"
        return "rows" if self.seedl <= 32 else "wide rows"

    @property
    def window(self) -> int:
        return self.max_ins - self.min_ins + 1

    @property
    def prm(self):
        return gc.default_params(self.totalkmax, max_gap=self.max_gap, min_flank=self.min_flank, margin=self.margin, max_cost=self.max_cost)

    @property
    def searched(self) -> bool:
        """does the gap stage search a read of this length at all"""
        return 2 * self.min_flank + self.max_gap + 1 <= self.patl


def draw(kind: str, seed: int) -> Config:
    rng = np.random.default_rng([KINDS[kind], seed])
    pick = lambda values: values[int(rng.integers(0, len(values)))]      # noqa: E731
    seedl = int(pick(SEEDLS))
    size = int(rng.integers(100_000, 200_001))
    table_kind = int(pick(TABLE_KINDS))
    if seedl == 32 and table_kind == 3:
        table_kind = 2                                                    # (rows of 32-base seeds need 2^28 rows)
    prefix_bits = 0
    if table_kind == 3:                                                   # fuzz_parity.py's rule
        lg = max(int(np.log2(size)), 2)
        r = int(rng.integers(1, 5))
        prefix_bits = min(seedl - 32, max(2, lg - r)) if seedl > 32 else min(30, max(1, seedl - r))
    totalkmax = int(rng.integers(1, 7))
    seedkmax = min(int(rng.integers(0, 3)), totalkmax)
    max_gap, min_flank = int(rng.integers(1, 17)), int(rng.integers(1, 13))
    n_files = int(rng.integers(1, 3))
    ids = [int(x) for x in rng.permutation(len(FILE_IDS))[:n_files]]
    common = dict(
        kind=kind, seed=int(seed), seedl=seedl, table_kind=table_kind, prefix_bits=int(prefix_bits), seedkmax=seedkmax, totalkmax=totalkmax,
        scores=int(rng.integers(0, 2)), filter_level=int(pick(FILTER_LEVELS)),
        qual_const=int(rng.integers(0, 64)) if rng.integers(0, 4) == 0 else None,
        size=size, n_frag=int(rng.integers(2, 9)), n_runs=int(rng.integers(0, 7)), fileids=tuple(FILE_IDS[i] for i in ids),
        max_gap=max_gap, min_flank=min_flank, margin=int(pick(MARGINS)),
        max_cost=None if rng.integers(0, 2) else int(rng.integers(6 + max_gap, 4 * totalkmax + 6 + max_gap + 1)),
        pileup_minq=int(pick(PILEUP_MINQ)), min_call_qual=int(pick(MIN_CALL_QUAL)), min_depth=int(pick(MIN_DEPTH)), min_alt=int(pick(MIN_ALT)),
        dedup_minq=int(pick(DEDUP_MINQ)), dedup=int(rng.integers(0, 2)), hist_bins=int(pick(HIST_BINS)),
        presentation=str(pick(PRESENTATIONS)), garbage_out=int(rng.integers(0, 2)), cut=str(pick(CUTS)), cut_frac=float(rng.random()),
        gapped_first=int(rng.integers(0, 2)), second_half_first=int(rng.integers(0, 2)),
        patl=int(pick(TARGET_LENGTHS)), n=int(rng.integers(65, 151)))
    if kind == "paired":
        anchor_l = int(pick(ANCHOR_MATE_LENGTHS))
        frag_l = common["patl"] + anchor_l + int(rng.integers(20, 121))
        window = int(pick(WINDOWS)) if rng.integers(0, 2) else int(rng.integers(2, 601))      # (wide enough for class R's second copy beside a 320-base target)
        max_ins = frag_l + window - 1
        assert max_ins <= MATE_SEARCH_MAX_INSERT
        return Config(**common, anchor_l=anchor_l, frag_l=frag_l, min_ins=frag_l, max_ins=max_ins, mate_search=int(rng.integers(0, 2)),
                      search_anchors=int(pick(SEARCH_ANCHORS)))
    # (the single-end plants copy the locus of class C forty times: long reads need the upper half of the size range)
    common["size"] = max(size, 100_000 + 300 * common["patl"])
    lo = max(seedl, 32)
    hi = max(lo, (common["patl"] - max_gap) // 2)
    return Config(**common, anchor_len=int(rng.integers(lo, hi + 1)), max_anchors=int(pick(SINGLE_ANCHORS)), n_blocks=int(rng.integers(1, 4)))


# ---- the workload -----------------------------------------------------------------------------------------------------------
def _quality(cfg: Config, stream: int):
    """the quality generator of one batch: a function length -> the qualities of the next read"""
    if cfg.qual_const is not None:
        return lambda length: np.full(length, cfg.qual_const, dtype=np.uint8)
    rng = np.random.default_rng([KINDS[cfg.kind], cfg.seed, 7, stream])

    def gen(length):
        q = rng.integers(0, 64, size=length).astype(np.uint8)
        if length > 8 and rng.integers(0, 4) == 0:                        # a run of quality 0
            s = int(rng.integers(0, length - 4))
            q[s:s + int(rng.integers(1, max(2, length // 4)))] = 0
        return q
    return gen


def n_copies(i: int) -> int:
    """the PCR copies of fragment / read i: three of every seventh, one of every seventh"""
    return 3 if i % 7 == 0 else 1 if i % 7 == 3 else 0


def _reads_of(b):
    return [(b.read(i).copy(), b.qual[int(b.offsets[i]):int(b.offsets[i + 1])].copy()) for i in range(b.n_reads)]


def _batch(rows, prefix):
    return gw.Batch([r for r, _ in rows], ["%s%d" % (prefix, i) for i in range(len(rows))],
                    np.concatenate([q for _, q in rows]) if rows else np.zeros(0, np.uint8))


_WORK = {}


def workload(cfg: Config):
    """-> namespace: files [(fileid, synth.Genome)] in the order of the run, the main file last; b1, b2 (paired) or b (single);
    n; cut (the split point of the configuration); plants (of the main file's workload)"""
    key = (cfg.kind, cfg.seed)
    if key in _WORK:
        return _WORK[key]
    ws = 1000 * (cfg.seed + 1) + KINDS[cfg.kind]
    geometry = dict(patl=cfg.patl, prm=cfg.prm, per_class=4, seedl=cfg.seedl, n_frag=cfg.n_frag, n_runs=cfg.n_runs)
    if cfg.kind == "paired":
        geometry.update(min_ins=cfg.min_ins, max_ins=cfg.max_ins, frag_l=cfg.frag_l, anchor_l=cfg.anchor_l)
        main = gw.workload(seed=ws, n=cfg.n, size=cfg.size, fileid=cfg.fileids[-1], qual=_quality(cfg, 0), **geometry)
        rows1, rows2 = _reads_of(main["b1"]), _reads_of(main["b2"])
        files = [(cfg.fileids[-1], main["g"])]
        if len(cfg.fileids) == 2:
            other = gw.workload(seed=ws + 1, n=20, size=100_000, fileid=cfg.fileids[0], qual=_quality(cfg, 1), **dict(geometry, per_class=1))
            rows1, rows2 = rows1 + _reads_of(other["b1"]), rows2 + _reads_of(other["b2"])
            files.insert(0, (cfg.fileids[0], other["g"]))
        q = _quality(cfg, 2)
        for i in range(len(rows1)):
            for _ in range(n_copies(i)):
                rows1.append((rows1[i][0].copy(), q(len(rows1[i][0]))))
                rows2.append((rows2[i][0].copy(), q(len(rows2[i][0]))))
        w = types.SimpleNamespace(files=files, b1=_batch(rows1, "f"), b2=_batch(rows2, "f"), plants=main["plants"])
        w.n = w.b1.n_reads
    else:
        main = aw.workload(seed=ws, n=cfg.n, size=cfg.size, fileid=cfg.fileids[-1], qual=_quality(cfg, 0), **geometry)
        rows = _reads_of(main["b"])
        files = [(cfg.fileids[-1], main["g"])]
        if len(cfg.fileids) == 2:
            other = aw.workload(seed=ws + 1, n=20, size=100_000, fileid=cfg.fileids[0], qual=_quality(cfg, 1), **dict(geometry, per_class=1))
            rows = rows + _reads_of(other["b"])
            files.insert(0, (cfg.fileids[0], other["g"]))
        q = _quality(cfg, 2)
        n_base = len(rows)
        for i in range(n_base):
            for _ in range(n_copies(i)):
                rows.append((rows[i][0].copy(), q(len(rows[i][0]))))
        if cfg.patl > sgw.CUT:                                            # single_gapped_workloads' cut copies: the same 5' end, a shorter span
            for i in range(5, n_base, 15):
                rows.append((rows[i][0][:sgw.CUT].copy(), rows[i][1][:sgw.CUT].copy()))
        w = types.SimpleNamespace(files=files, b=_batch(rows, "r"), plants=main["plants"])
        w.n = w.b.n_reads
    w.cut = 0 if cfg.cut == "zero" else w.n if cfg.cut == "all" else 1 + int(cfg.cut_frac * (w.n - 1))
    w.main_fid, w.main = files[-1]
    _WORK[key] = w
    return w


def workload_digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digest_of(cfg: Config) -> str:
    w = workload(cfg)
    parts = []
    for b in ((w.b1, w.b2) if cfg.kind == "paired" else (w.b,)):
        parts += [b.bases, b.qual, b.offsets]
    for _, g in w.files:
        parts += [g.sym, np.asarray(g.frag_start, dtype=np.uint64)]
    return workload_digest(*parts)


# ---- differences ------------------------------------------------------------------------------------------------------------
class StageDiff(AssertionError):
    def __init__(self, stage, cfg, why):
        super().__init__("stage %s differs for %r: %s" % (stage, cfg, why))
        self.stage, self.cfg = stage, cfg


def _same_bytes(got, want, what):
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape[0] == w.shape[0], "%s: %d against %d records" % (what, g.shape[0], w.shape[0])
    if g.dtype != w.dtype and g.dtype.kind in "iu" and w.dtype.kind in "iu":      # (the checkers count in int64: the values, whole)
        bad = np.nonzero(g.astype(np.int64).reshape(-1) != w.astype(np.int64).reshape(-1))[0]
        assert bad.size == 0, "%s differs at %d places, first %d: got %d want %d" % (what, bad.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])
        return
    if g.dtype.names and w.dtype.names and set(g.dtype.names) >= set(w.dtype.names):      # records: field by field, the first one named
        for f in w.dtype.names:
            a, b = np.asarray(g[f]), np.asarray(w[f])
            if a.dtype.kind == "f":
                a, b = a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64), b.view(np.uint32 if b.dtype.itemsize == 4 else np.uint64)
            bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0] if a.shape[0] else np.zeros(0, np.int64)
            assert bad.size == 0, "%s field %s differs at %d records, first %d: got %r want %r" % (what, f, bad.size, bad[0], got[bad[0]], want[bad[0]])
    if g.dtype.names is None and w.dtype.names is None and g.dtype == w.dtype and g.tobytes() != w.tobytes():
        bad = np.nonzero(g.reshape(-1) != w.reshape(-1))[0]
        assert bad.size == 0, "%s differs at %d places, first %d: got %r want %r" % (what, bad.size, bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]])
    assert g.tobytes() == w.tobytes(), "%s: the bytes of %d records differ" % (what, g.shape[0])


def _same_lists(got, want, what):
    """mismatch lists: the entries up to the last offset, field by field"""
    assert got.shape[0] >= want.shape[0], (what, got.shape, want.shape)
    for f in ("off", "ref", "base"):
        bad = np.nonzero(np.asarray(got[f][:want.shape[0]]) != np.asarray(want[f]))[0]
        assert bad.size == 0, "%s field %s differs at %d entries, first %d" % (what, f, bad.size, bad[0])


# the assert helper of every named output; every other array is compared whole, byte for byte, every dictionary counter by counter
HELPERS = {"pairs": pc.assert_records_equal, "singles1": sc.assert_singles_equal, "singles2": sc.assert_singles_equal,
           "gaps": gc.assert_records_equal, "events": ic.assert_lists_equal, "indel_calls": ic.assert_lists_equal, "lists": _same_lists}


def check_stage(cfg: Config, stage: str, got: dict, want: dict, what: str = "whole"):
    """every output of a stage against the expected one; StageDiff names the stage and the configuration"""
    try:
        assert set(got) == set(want), (sorted(got), sorted(want))
        for key, w in want.items():
            g = got[key]
            if key.startswith("pair_hits"):
                pac.assert_pair_hits_equal(g, w, "%s %s" % (what, key))
            elif key in HELPERS:
                HELPERS[key](g, w, "%s %s" % (what, key))
            elif isinstance(w, dict):
                assert {k: int(g[k]) for k in w} == {k: int(v) for k, v in w.items()}, "%s %s: got %r want %r" % (what, key, {k: int(g[k]) for k in w}, w)
            else:
                _same_bytes(g, w, "%s %s" % (what, key))
    except AssertionError as e:
        if isinstance(e, StageDiff):
            raise
        raise StageDiff(stage, cfg, e) from e


# ---- expected ---------------------------------------------------------------------------------------------------------------
_EXPECTED = {}


def expected(cfg: Config, ora) -> dict:
    key = (cfg.kind, cfg.seed)
    if key not in _EXPECTED:
        _EXPECTED[key] = (_expected_paired if cfg.kind == "paired" else _expected_single)(cfg, ora)
    return _EXPECTED[key]


def _lens(b):
    return np.diff(b.offsets.astype(np.int64))


def _params(cfg, ora, fid):
    return ora.make_params(seedl=cfg.seedl, seedkmax=cfg.seedkmax, totalkmax=cfg.totalkmax, scores=cfg.scores, filter_level=cfg.filter_level, fileid=fid)


def _consumers(cfg, w, mates, gaps, add_ungapped):
    """the pileup, the calls and the indel calls of the main file: add_ungapped(stage) makes the ungapped add"""
    sym, fid = w.main.sym, w.main_fid
    pu = pgc.GappedPileup(sym, fid, cfg.pileup_minq)
    add_ungapped(pu)
    pu.add_gapped(*mates, gaps)
    cl = pgc.GappedCalls(pu)
    add_ungapped(cl)
    cl.add_gapped(*mates, gaps)
    ind = ic.Indels(pu.ungapped_view(), w.main.frag_start)
    ind.add(*mates, gaps)
    thr_c, thr_i = (cfg.min_call_qual, cfg.min_depth), (cfg.min_call_qual, cfg.min_alt, cfg.min_depth)
    return {
        "pileup": dict(depth=pu.depth, gdepth=pu.gdepth, sites=pu.sites(), stats=pu.finish_stats(), gstats=pu.gapped_stats()),
        "calls": dict(evidence=cl.evidence(), calls=cl.calls(*thr_c), stats=cl.finish_stats(*thr_c), gstats=dict(cl.gstats)),
        "indels": dict(events=ind.events(*thr_i), indel_calls=ind.calls(*thr_i), stats=ind.finish_stats(*thr_i))}


def _expected_paired(cfg, ora):
    w = workload(cfg)
    b1, b2, n = w.b1, w.b2, w.n
    l1, l2 = _lens(b1), _lens(b2)
    fm = ora.filter_mult(cfg.filter_level, cfg.totalkmax)
    scores = bool(cfg.scores)
    files = []
    for fid, g in w.files:
        og = ora.Genome(g.sym, g.frag_start)
        ix = ora.Index(og, cfg.seedl)
        p = _params(cfg, ora, fid)
        h1, o1, _ = ora.match_all(og, ix, p, b1.bases, b1.qual, b1.offsets)
        h2, o2, _ = ora.match_all(og, ix, p, b2.bases, b2.qual, b2.offsets)
        files.append((fid, h1, o1, h2, o2))
    exp = {}
    plain = pc.check_pairs(files, l1, l2, cfg.min_ins, cfg.max_ins, scores, fm)
    first = dict(singles1=sc.check_singles([(f[0], f[1], f[2]) for f in files], l1, scores, fm),
                 singles2=sc.check_singles([(f[0], f[3], f[4]) for f in files], l2, scores, fm))
    if cfg.mate_search:
        pairs, ctr = mc.check_pairs_search(ora, dict(w.files), files, b1, b2, cfg.min_ins, cfg.max_ins, scores, fm, cfg.seedl, cfg.totalkmax,
                                           cfg.search_anchors)
        first.update(pairs=pairs, search_stats=ctr)
    else:
        pairs = plain
        first.update(pairs=pairs)
    exp["match_pairs_singles"] = first
    exp["_plain_pairs"], exp["_files"] = plain, files
    s1, s2 = first["singles1"], first["singles2"]
    every = {}
    for fid, h1, o1, h2, o2 in files:
        recs, off = pac.enumerate_pairs(h1, o1, l1, h2, o2, l2, cfg.min_ins, cfg.max_ins, fid)
        every["pair_hits_%d" % fid], every["pair_offsets_%d" % fid] = recs, off
        every["stats_%d" % fid] = pac.expected_stats(o1, o2, recs)
    exp["match_pairs_all"] = every
    hist, hstats = ik.histogram(pairs, l1, l2, cfg.hist_bins)
    exp["insert_hist"] = dict(hist=hist, stats=hstats)
    accp = mq.check_pair_hits([f[1:] for f in files], l1, l2, cfg.min_ins, cfg.max_ins, scores)
    acc1, acc2 = mq.check_hits([(f[1], f[2]) for f in files], n, scores), mq.check_hits([(f[3], f[4]) for f in files], n, scores)
    q, placed, unl = mq.finish_pairs(pairs, s1, s2, accp, acc1, acc2, scores)
    exp["mapq"] = dict(acc_pair=mq.acc_records(accp), acc1=mq.acc_records(acc1), acc2=mq.acc_records(acc2), mapq=q,
                       finish=dict(placements=placed, unlisted=unl))
    sums1, sums2 = dk.summaries_of(b1, cfg.dedup_minq), dk.summaries_of(b2, cfg.dedup_minq)
    dup, dstats, _ = dk.mark_pairs(pairs, sums1, sums2)
    exp["duplicates"] = dict(sums1=sums1, sums2=sums2, dup=dup, stats=dstats)
    lists, off, st = sk.mismatch_lists(w.main.sym, w.main_fid, sk.final_pairs(pairs, s1, s2), sk.pair_reads(b1, b2))
    exp["mismatches_pairs"] = dict(lists=lists, offsets=off, stats=st)
    gaps, gap = None, {}
    for fid, g in w.files[::-1]:                                          # the resident file first, then the other folds into it
        gaps, ctr = gc.check_gap(gc.Text(g.sym, g.frag_start, fid), b1, b2, pairs, s1, s2, cfg.min_ins, cfg.max_ins, cfg.prm, out=gaps)
        gap["stats_%d" % fid] = ctr
    exp["gap_rescue"] = dict(gap, gaps=gaps)
    lists, off, st = glc.gapped_lists(w.main.sym, w.main_fid, b1, b2, gaps)
    exp["mismatches_gapped"] = dict(lists=lists, offsets=off, stats=st)
    placed_pairs = dk.masked_pairs(pairs, dup) if cfg.dedup else pairs
    exp.update(_consumers(cfg, w, (b1, b2), gaps, lambda stage: stage.add_pairs(b1, b2, placed_pairs)))
    return exp


def per_block(cfg: Config, g) -> int:
    """index entries per block: the text's windows in n_blocks blocks"""
    return (1 << 62) if cfg.n_blocks == 1 else int(g.n) // cfg.n_blocks + 1


def _expected_single(cfg, ora):
    w = workload(cfg)
    b, n = w.b, w.n
    scores = bool(cfg.scores)
    sub = gac.SubBatch(b, cfg.anchor_len)
    info = score = None
    blocks = []
    counters = None
    for fid, g in w.files:
        og = ora.Genome(g.sym, g.frag_start)
        p = _params(cfg, ora, fid)
        first = 0
        while True:
            ix = ora.Index(og, cfg.seedl, first, per_block(cfg, g))
            info, score, ctr = ora.match_unique(og, ix, p, b.bases, b.qual, b.offsets, info=info, score=score)
            counters = ctr if counters is None else {k: counters[k] + ctr[k] for k in ctr}
            hf, of, _ = ora.match_all(og, ix, p, b.bases, b.qual, b.offsets)
            hs, os_, _ = ora.match_all(og, ix, p, sub.bases, sub.qual, sub.offsets)
            blocks.append((fid, g, hf, of, hs, os_))
            first += ix.n
            if not ix.have_next:
                break
    exp = {"_blocks": len(blocks), "_lists": blocks}
    first = dict(info=info.copy(), counters={k: counters[k] for k in ("reads", "lookups", "candidates", "seedpass", "hits")})
    if scores:
        first["score"] = score.copy().view(np.uint32)
    exp["match_unique"] = first
    accs = mq.check_hits([(x[2], x[3]) for x in blocks], n, scores)
    state, _, err, _, _ = ora.unpack_record(info)
    q, placed, unl = mq.finish_single(state, err, score, accs, scores)
    exp["mapq"] = dict(acc=mq.acc_records(accs), mapq=q, finish=dict(placements=placed, unlisted=unl))
    ap = gac.AnchorParams(cfg.anchor_len, cfg.max_anchors)
    gaps, total = None, dict.fromkeys(gac.COUNTERS, 0)
    for fid, g, _, _, hs, os_ in blocks:
        gaps, ctr = gac.check_anchor(gc.Text(g.sym, g.frag_start, fid), b, info, hs, os_, cfg.prm, ap, out=gaps)
        total = {k: total[k] + ctr[k] for k in total}
    exp["match_gapped"] = dict(gaps=gaps, stats=total)
    sums = dk.summaries_of(b, cfg.dedup_minq)
    dup1, st1, _ = dk.mark_single(info, sums)
    dupg, stg, _ = dgk.mark_groups(info, gaps, sums)
    exp["duplicates"] = dict(sums=sums, dup=dup1, stats=st1, dup_gapped=dupg, stats_gapped=stg)
    lists, off, st = sk.mismatch_lists(w.main.sym, w.main_fid, sk.final_single(info, score), sk.single_reads(b))
    exp["mismatches"] = dict(lists=lists, offsets=off, stats=st)
    lists, off, st = glc.gapped_lists(w.main.sym, w.main_fid, b, b, gaps)
    exp["mismatches_gapped"] = dict(lists=lists, offsets=off, stats=st)
    placed_info = dk.masked_info(info, dupg) if cfg.dedup else info
    placed_gaps = dgk.masked_gaps(gaps, dupg) if cfg.dedup else gaps
    exp.update(_consumers(cfg, w, (b, b), placed_gaps, lambda stage: stage.add(b, placed_info)))
    return exp


# ---- the same chains on the device -------------------------------------------------------------------------------------------
class PackedMate:
    """a batch with 2-bit bases whose first read starts inside a byte: one base in front of everything, the offsets moved by it"""
    def __init__(self, b):
        from real_amd import synth
        self.bases = synth.pack_bases(np.concatenate([np.zeros(1, np.uint8), b.bases]))
        self.qual = np.concatenate([np.zeros(1, np.uint8), b.qual])
        self.offsets = (b.offsets + np.uint64(1)).astype(np.uint64)
        self.nflags = synth.read_nflags(b.bases, b.offsets)


def make_matcher(cfg: Config):
    """the default matcher_factory: one PairMatcher context with the configuration's matcher parameters and index layout"""
    from real_amd.matcher import PairMatcher, RealOptions

    class Matcher(PairMatcher):
        def _mate_batch(self, mate, **kw):
            if isinstance(mate, PackedMate):
                return self._read_batch(mate.bases, mate.qual, mate.offsets, packed=True, nflags=mate.nflags, **kw)
            return super()._mate_batch(mate, **kw)
    opts = RealOptions(seedl=cfg.seedl, seedkmax=cfg.seedkmax, totalkmax=cfg.totalkmax, scores=bool(cfg.scores), filter_level=cfg.filter_level).normalise()
    return Matcher(opts, prefix_bits=cfg.prefix_bits, table_kind=cfg.table_kind)


class _Presenter:
    """how a configuration hands its arrays over"""
    def __init__(self, cfg):
        self.mode, self.garbage = cfg.presentation, bool(cfg.garbage_out)
        self.device_reads = self.mode in ("device", "mixed")
        self.device_records = self.mode == "device"
        self.empty = []                     # the output tensors of empty calls

    @staticmethod
    def to_device(a):
        import torch
        a = np.ascontiguousarray(a)
        n = int(a.shape[0])
        if n == 0:                                                        # (an empty tensor has no address: the empty head of one record)
            a = np.zeros(1, dtype=a.dtype)
        if a.dtype == np.uint64:
            return torch.from_numpy(a.view(np.int64).copy()).cuda()[:n]
        if a.dtype.itemsize > 1 or a.dtype.names:
            return torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], a.dtype.itemsize).copy()).cuda()[:n]
        return torch.from_numpy(a.copy()).cuda()[:n]

    def mate(self, b):
        """a batch as the stages take it through _mate_batch"""
        if self.device_reads:
            import torch
            return tuple(self.to_device(x) for x in (b.bases, b.qual, b.offsets))
        return PackedMate(b) if self.mode == "packed" else b

    def flat(self, b, packed_ok=True):
        """-> (bases, qual), keywords: a batch for the stages that take the three arrays one by one"""
        m = self.mate(b) if (packed_ok or self.mode != "packed") else b
        if isinstance(m, PackedMate):
            return (m.bases, m.qual), dict(offsets=m.offsets, packed=True, nflags=m.nflags)
        if isinstance(m, tuple):
            return m[:2], dict(offsets=m[2])
        return (m.bases, m.qual), dict(offsets=m.offsets)

    def records(self, a):
        """input records: where the presentation keeps them"""
        return self.to_device(a) if self.device_records else a

    def output(self, n, dtype, force_device=False):
        """an output array: None (the wrapper makes a fresh one), or one filled with garbage; on the device where the stage needs it there"""
        dtype = np.dtype(dtype)
        if self.device_records or force_device:
            import torch
            room = max(n, 1)            # (an empty tensor has no address and the matcher's entry points refuse NULL: room for one record)
            if dtype == np.uint64:
                t = torch.full((room,), 0x7123456789abcdef if self.garbage else 0, dtype=torch.int64, device="cuda")
            elif dtype == np.float32:
                t = torch.full((room,), 1e30 if self.garbage else 0.0, dtype=torch.float32, device="cuda")
            else:
                t = torch.full((room, dtype.itemsize), 0xAB if self.garbage else 0, dtype=torch.uint8, device="cuda")
            if n == 0:
                self.empty.append(t)
            return t
        if not self.garbage:
            return None
        return np.full(n * dtype.itemsize, 0xAB, dtype=np.uint8).view(dtype)

    def host(self, x, dtype):
        if x is None or isinstance(x, np.ndarray):
            return x
        if any(x is t for t in self.empty):
            return np.zeros(0, dtype=dtype)
        return np.ascontiguousarray(x.cpu().numpy()).reshape(-1).view(np.uint8).view(dtype)


def _counters(st, names):
    return {k: int(st[k]) for k in names}


class _Run:
    def __init__(self, cfg, ora, make):
        self.cfg, self.exp, self.w = cfg, expected(cfg, ora), workload(cfg)
        self.P = _Presenter(cfg)
        self.m = make(cfg)
        n, c = self.w.n, self.w.cut
        self.spans = [(0, n), (0, c), (c, n)]
        self.launches = {}

    def check(self, stage, got, what="whole"):
        check_stage(self.cfg, stage, got, self.exp[stage], what)

    def note(self, stage, stats):
        """the kernels a stage launched, from its statistics (real_hip_pair_stats and the matcher's counters have no such field:
        the join and match_unique are not noted)"""
        self.launches[stage] = self.launches.get(stage, 0) + int(stats["launches"])

    def joined(self, parts):
        return np.concatenate(parts)

    def lists_joined(self, parts):
        """(lists, offsets) of two calls as those of one"""
        (la, oa), (lb, ob) = parts
        na = int(oa[-1])
        return np.concatenate([la[:na], lb[:int(ob[-1])]]), np.concatenate([oa, ob[1:] + oa[-1]])

    def adds(self, kinds=("ungapped", "gapped")):
        """the order of the adds of an accumulating stage run in halves"""
        order = [(k, s) for k in (kinds[::-1] if self.cfg.gapped_first else kinds) for s in ((2, 1) if self.cfg.second_half_first else (1, 2))]
        return [(k, self.spans[s]) for k, s in order]

    def finish(self):
        missing = [k for k, v in self.launches.items() if v <= 0]
        if missing:
            raise StageDiff(",".join(missing), self.cfg, "no kernel was launched")

    # -- the consumers both chains end with --
    def consumers(self, mates_of, gaps, add_ungapped, call_add_ungapped):
        """pileup, calls and indel calls: mates_of(lo, hi) -> the two batches, gaps the host records, add_ungapped(lo, hi) makes the
        pileup's ungapped add of that span, call_add_ungapped the calls'"""
        cfg, m, P = self.cfg, self.m, self.P
        n = self.w.n
        size = int(self.w.main.sym.shape[0])
        thr_c, thr_i = (cfg.min_call_qual, cfg.min_depth), (cfg.min_call_qual, cfg.min_alt, cfg.min_depth)
        plans = {"whole": [("ungapped", (0, n)), ("gapped", (0, n))], "halves": self.adds()}
        if cfg.gapped_first:
            plans["whole"].reverse()
        for what, plan in plans.items():
            for reset in (m.pileup_stats, m.call_stats, m.pileup_gapped_stats, m.indel_stats):
                reset(reset=True)
            m.pileup_begin(cfg.pileup_minq)
            for kind, (lo, hi) in plan:
                if kind == "ungapped":
                    add_ungapped(lo, hi)
                else:
                    m.pileup_add_gapped(*mates_of(lo, hi), P.records(gaps[lo:hi]))
            m.pileup_finish()
            st, gst = m.pileup_stats(), m.pileup_gapped_stats(reset=True)
            want = self.exp["pileup"]
            self.check("pileup", dict(depth=m.pileup_depth(0, size), gdepth=m.pileup_depth_gapped(0, size), sites=m.pileup_sites(),
                                      stats=_counters(st, want["stats"]), gstats=_counters(gst, want["gstats"])), what)
            self.note("pileup", st)
            self.note("pileup_gapped", gst)
            m.call_begin()
            for kind, (lo, hi) in plan:
                if kind == "ungapped":
                    call_add_ungapped(lo, hi)
                else:
                    m.call_add_gapped(*mates_of(lo, hi), P.records(gaps[lo:hi]))
            m.call_finish(*thr_c)
            st, gst = m.call_stats(), m.pileup_gapped_stats()
            want = self.exp["calls"]
            self.check("calls", dict(evidence=m.call_evidence(), calls=m.call_variants(), stats=_counters(st, want["stats"]),
                                     gstats=_counters(gst, want["gstats"])), what)
            self.note("calls", st)
            self.note("calls_gapped", gst)
            m.indel_begin()
            for kind, (lo, hi) in plan:
                if kind == "gapped":
                    m.indel_add(*mates_of(lo, hi), P.records(gaps[lo:hi]))
            m.indel_finish(*thr_i)
            st = m.indel_stats()
            self.check("indels", dict(events=m.indel_events(), indel_calls=m.indel_calls(), stats=_counters(st, self.exp["indels"]["stats"])), what)
            self.note("indels", st)
            m.indel_end()
            m.call_end()
            m.pileup_end()

    def gapped_lists(self, mates_of, gaps):
        m, P = self.m, self.P
        want = self.exp["mismatches_gapped"]
        got = []
        for k, (lo, hi) in enumerate(self.spans):
            if k < 2:
                m.gapped_list_stats(reset=True)
            lists, off = m.mismatches_gapped(*mates_of(lo, hi), P.records(gaps[lo:hi]))
            got.append((P.host(lists, sk.MM_DTYPE), P.host(off, np.uint64)))
            if k != 1:
                st = m.gapped_list_stats()
                lists, off = got[0] if k == 0 else self.lists_joined(got[1:])
                self.check("mismatches_gapped", dict(lists=lists, offsets=off, stats=_counters(st, want["stats"])), "whole" if k == 0 else "halves")
                self.note("mismatches_gapped", st)


def _run_paired(R: _Run):
    cfg, m, P, w, exp = R.cfg, R.m, R.P, R.w, R.exp
    from real_amd import lib as rlib
    b1, b2, n = w.b1, w.b2, w.n
    l1, l2 = _lens(b1).astype(np.uint32), _lens(b2).astype(np.uint32)
    spans = R.spans
    parts = [(b1.part(lo, hi), b2.part(lo, hi)) for lo, hi in spans]
    mates = [(P.mate(a), P.mate(b)) for a, b in parts]
    by_span = dict(zip(spans, mates))

    def mates_of(lo, hi):
        return by_span[(lo, hi)]
    search = dict(mate_search=bool(cfg.mate_search), max_anchors=cfg.search_anchors)
    ins = (cfg.min_ins, cfg.max_ins)
    sizes = (rlib.PAIR_DTYPE, rlib.SINGLE_DTYPE, rlib.SINGLE_DTYPE, rlib.MAPQ_ACC_DTYPE, rlib.MAPQ_ACC_DTYPE, rlib.MAPQ_ACC_DTYPE)
    # 1, 2, 4: the stages that need the index, file by file; the records of the first file fold into the second pass
    recs = [None] * 3
    recq = [None] * 3
    every, every_stats = {}, {}
    searched = [[dict.fromkeys(mc.COUNTERS, 0) for _ in spans] for _ in range(2)]     # per entry point, per run: summed over the files

    def count_search(entry, k):
        if not cfg.mate_search:
            return
        st = m.mate_search_stats(reset=True)
        R.note("mate_search", st)
        for name in mc.COUNTERS:
            searched[entry][k][name] += int(st[name])
    for stats in (m.pair_stats, m.single_stats, m.mate_search_stats, m.pair_all_stats, m.mapq_stats):
        stats(reset=True)
    for fi, (fid, g) in enumerate(w.files):
        m.set_text_symbols(fid, g.sym, g.frag_start)
        m.build_index_block()
        for k, (lo, hi) in enumerate(spans):
            if fi == 0:
                outs = [P.output(hi - lo, d, force_device=P.device_reads) for d in sizes]
                fresh = None if outs[0] is None else True
                recs[k] = m.match_pairs_singles(*mates[k], *ins, *outs[:3], fresh=fresh, **search)
                count_search(0, k)
                outs = [P.output(hi - lo, d, force_device=P.device_reads) for d in sizes]
                recq[k] = m.match_pairs_mapq(*mates[k], *ins, *outs, fresh=fresh, **search)
                count_search(1, k)
            else:
                recs[k] = m.match_pairs_singles(*mates[k], *ins, *recs[k], fresh=False, **search)
                count_search(0, k)
                recq[k] = m.match_pairs_mapq(*mates[k], *ins, *recq[k], fresh=False, **search)
                count_search(1, k)
        # every concordant pair of this file: the whole batch and the halves
        got, got_stats = [], []
        for k, (lo, hi) in enumerate(spans):
            m.pair_all_stats(reset=True)
            if P.device_reads:
                import torch
                cap = int(exp["match_pairs_all"]["pair_hits_%d" % fid].shape[0]) + 1
                out = torch.full((cap, 32), 0xAB if P.garbage else 0, dtype=torch.uint8, device="cuda")
                poff = torch.zeros(hi - lo + 1, dtype=torch.int64, device="cuda")
                count, _ = m.match_pairs_all(*mates[k], *ins, out=out, pair_offsets=poff)
                got.append((P.host(out, rlib.PAIR_HIT_DTYPE)[:count], P.host(poff, np.uint64)))
            else:
                got.append(m.match_pairs_all(*mates[k], *ins))
            st = m.pair_all_stats()
            R.note("match_pairs_all", st)
            got_stats.append(_counters(st, ("products", "pairs_out", "handed_over")))
        (ra, oa), (rb, ob) = got[1], got[2]
        rb = rb.copy()
        rb["pair"] += np.uint32(spans[1][1])
        every[fid] = (got[0], (np.concatenate([ra, rb]), np.concatenate([oa, ob[1:] + oa[-1]])))
        every_stats[fid] = (got_stats[0], {name: got_stats[1][name] + got_stats[2][name] for name in got_stats[0]})
    host = [[P.host(x, d) for x, d in zip(r, sizes)] for r in recs]
    hostq = [[P.host(x, d) for x, d in zip(r, sizes)] for r in recq]
    for what, pick in (("whole", lambda h: h[0]), ("halves", lambda h: [R.joined([a, b]) for a, b in zip(h[1], h[2])])):
        r, rq = pick(host), pick(hostq)
        got = dict(pairs=r[0], singles1=r[1], singles2=r[2])
        k = 0 if what == "whole" else 1
        same = dict(pairs=exp["match_pairs_singles"]["pairs"], singles1=exp["match_pairs_singles"]["singles1"], singles2=exp["match_pairs_singles"]["singles2"])
        gotq = dict(pairs=rq[0], singles1=rq[1], singles2=rq[2])
        if cfg.mate_search:                                               # the search's counters of this run, of either entry point
            for entry, d in ((0, got), (1, gotq)):
                runs = searched[entry]
                d["search_stats"] = runs[0] if k == 0 else {name: runs[1][name] + runs[2][name] for name in mc.COUNTERS}
            same["search_stats"] = exp["match_pairs_singles"]["search_stats"]
        R.check("match_pairs_singles", got, what)
        check_stage(cfg, "match_pairs_mapq", gotq, same, what)
        R.check("match_pairs_all", dict([("pair_hits_%d" % fid, every[fid][k][0]) for fid in every] + [("pair_offsets_%d" % fid, every[fid][k][1]) for fid in every] +
                                        [("stats_%d" % fid, every_stats[fid][k]) for fid in every]), what)
    R.note("singles", m.single_stats())                                   # (real_hip_pair_stats has no launches field: the join is not noted)
    pairs, s1, s2 = host[0][:3]
    accs = hostq[0][3:]
    # 3: the insert histogram
    want = exp["insert_hist"]
    for what in ("whole", "halves"):
        m.insert_stats(reset=True)
        hist = None
        for lo, hi in ([spans[0]] if what == "whole" else (spans[2:0:-1] if cfg.second_half_first else spans[1:])):
            if hist is None:
                hist = P.output(cfg.hist_bins, np.uint64)
                fresh = None if hist is None else True
            else:
                fresh = False
            hist = m.insert_hist(P.records(pairs[lo:hi]), P.records(l1[lo:hi]) if P.device_records else l1[lo:hi],
                                 P.records(l2[lo:hi]) if P.device_records else l2[lo:hi], cfg.hist_bins, hist=hist, fresh=fresh)
        st = m.insert_stats()
        R.check("insert_hist", dict(hist=P.host(hist, np.uint64), stats=_counters(st, want["stats"])), what)
        R.note("insert_hist", st)
    # 4: the mapping quality: the accumulators of match_pairs_mapq, then the finish
    want = exp["mapq"]
    R.note("mapq", m.mapq_stats(reset=True))
    qs, fin = [], []
    for k, (lo, hi) in enumerate(spans):
        rq = hostq[k]
        q = m.mapq_pairs(*[P.records(x) for x in (rq[0], rq[3], rq[1], rq[2], rq[4], rq[5])])
        qs.append(P.host(q, np.uint8))
        fin.append(_counters(m.mapq_stats(reset=True), want["finish"]))
    halves = [R.joined([a, b]) for a, b in zip(hostq[1], hostq[2])]
    for what, rq, q, f in (("whole", hostq[0], qs[0], fin[0]), ("halves", halves, R.joined(qs[1:]), {name: fin[1][name] + fin[2][name] for name in fin[0]})):
        R.check("mapq", dict(acc_pair=rq[3], acc1=rq[4], acc2=rq[5], mapq=q, finish=f), what)
    # 5: read summaries and the marks (the marking is one call over all fragments: groups do not split)
    want = exp["duplicates"]
    m.dup_stats(reset=True)
    sums = []
    for b in (b1, b2):
        got = []
        for k, (lo, hi) in enumerate(spans):
            args, kw = P.flat(b.part(lo, hi))
            out = np.zeros(hi - lo, dtype=rlib.READ_SUM_DTYPE) if P.mode == "mixed" else None
            got.append(P.host(m.read_summary(*args, min_qual=cfg.dedup_minq, out=out, **kw), rlib.READ_SUM_DTYPE))
        _same_or_diff(cfg, "duplicates", got[0], R.joined(got[1:]), "the summaries of the halves")
        sums.append(got[0])
    dup = P.host(m.mark_duplicates_pairs(P.records(pairs), P.records(sums[0]), P.records(sums[1])), np.uint8)
    st = m.dup_stats()
    R.check("duplicates", dict(sums1=sums[0], sums2=sums[1], dup=dup, stats=_counters(st, want["stats"])))
    R.note("duplicates", st)
    # 6: the mismatch lists of the placed mates, on the main file (resident, the last one matched)
    want = exp["mismatches_pairs"]
    got = []
    for k, (lo, hi) in enumerate(spans):
        if k < 2:
            m.mismatch_stats(reset=True)
        lists, off = m.mismatches_pairs(*mates[k], P.records(pairs[lo:hi]), P.records(s1[lo:hi]), P.records(s2[lo:hi]))
        got.append((P.host(lists, sk.MM_DTYPE), P.host(off, np.uint64)))
        if k != 1:
            st = m.mismatch_stats()
            lists, off = got[0] if k == 0 else R.lists_joined(got[1:])
            R.check("mismatches_pairs", dict(lists=lists, offsets=off, stats=_counters(st, want["stats"])), "whole" if k == 0 else "halves")
            R.note("mismatches_pairs", st)
    # 7: gap rescue: the resident file starts the records, the other file folds into them (the text alone, no index)
    gaps = [None] * 3
    got_stats = {}
    for fi, (fid, g) in enumerate(w.files[::-1]):
        if fi:
            m.set_text_symbols(fid, g.sym, g.frag_start)
        for k, (lo, hi) in enumerate(spans):
            if k < 2:
                m.gap_stats(reset=True)
            if fi == 0:
                out = P.output(hi - lo, rlib.GAP_PLACE_DTYPE)
                fresh = None if out is None else True
            else:
                out, fresh = gaps[k], False
            gaps[k] = m.gap_rescue(*mates[k], P.records(pairs[lo:hi]), P.records(s1[lo:hi]), P.records(s2[lo:hi]), *ins, out=out, fresh=fresh,
                                   **cfg.prm._asdict())
            if k != 1:
                st = m.gap_stats()
                got_stats[(k, fid)] = _counters(st, gc.COUNTERS)
                R.note("gap_rescue", st)
    if len(w.files) == 2:
        m.set_text_symbols(w.main_fid, w.main.sym, w.main.frag_start)
    hg = [P.host(x, rlib.GAP_PLACE_DTYPE) for x in gaps]
    for what, k, rec in (("whole", 0, hg[0]), ("halves", 2, R.joined(hg[1:]))):
        R.check("gap_rescue", dict([("gaps", rec)] + [("stats_%d" % fid, got_stats[(k, fid)]) for fid, _ in w.files]), what)
    gaps = hg[0]
    # 8 .. 11
    R.gapped_lists(mates_of, gaps)
    placed = dk.masked_pairs(pairs, dup) if cfg.dedup else pairs
    R.consumers(mates_of, gaps, lambda lo, hi: m.pileup_add_pairs(*mates_of(lo, hi), P.records(placed[lo:hi])),
                lambda lo, hi: m.call_add_pairs(*mates_of(lo, hi), P.records(placed[lo:hi])))


def _same_or_diff(cfg, stage, got, want, what):
    try:
        _same_bytes(got, want, what)
    except AssertionError as e:
        raise StageDiff(stage, cfg, e) from e


def _run_single(R: _Run):
    cfg, m, P, w, exp = R.cfg, R.m, R.P, R.w, R.exp
    from real_amd import lib as rlib
    b, n = w.b, w.n
    spans = R.spans
    parts = [b.part(lo, hi) for lo, hi in spans]
    mates = [P.mate(x) for x in parts]
    by_span = {s: (x, x) for s, x in zip(spans, mates)}

    def mates_of(lo, hi):
        return by_span[(lo, hi)]
    scores = bool(cfg.scores)
    dev = P.device_reads
    # 1, 2: match_unique and the accumulators of the mapping quality over the files and their index blocks
    info, score, acc = [None] * 3, [None] * 3, [None] * 3
    ctr = [{} for _ in spans]                                             # the matcher's counters of every run, summed over the blocks
    m.mapq_stats(reset=True)
    blocks = []
    for fid, g in w.files:
        m.set_text_symbols(fid, g.sym, g.frag_start)
        first, more = 0, True
        while more:
            n_ent, more = m.build_index_block(first, per_block(cfg, g))
            for k, (lo, hi) in enumerate(spans):
                args, kw = P.flat(parts[k])
                margs, mkw = P.flat(parts[k], packed_ok=False)
                m.counters(reset=True)                                    # (the matcher's counters: those of match_unique alone)
                if not blocks:
                    info[k] = P.output(hi - lo, np.uint64, force_device=dev)
                    score[k] = P.output(hi - lo, np.float32, force_device=dev) if scores and info[k] is not None else None
                    acc[k] = P.output(hi - lo, rlib.MAPQ_ACC_DTYPE, force_device=dev)
                    info[k], score[k] = m.match_unique(*args, info=info[k], score=score[k], fresh=info[k] is not None, **kw)
                    ctr[k] = {key: ctr[k].get(key, 0) + v for key, v in m.counters().items()}
                    acc[k] = m.match_mapq(*margs, acc=acc[k], fresh=None if acc[k] is None else True, **mkw)
                else:
                    info[k], score[k] = m.match_unique(*args, info=info[k], score=score[k], **kw)
                    ctr[k] = {key: ctr[k].get(key, 0) + v for key, v in m.counters().items()}
                    acc[k] = m.match_mapq(*margs, acc=acc[k], fresh=False, **mkw)
            blocks.append((fid, first))
            first += n_ent
    assert len(blocks) == exp["_blocks"], (len(blocks), exp["_blocks"])
    hi_ = [P.host(x, np.uint64) for x in info]
    hs_ = [None if x is None else P.host(x, np.float32) for x in score]
    ha_ = [P.host(x, rlib.MAPQ_ACC_DTYPE) for x in acc]
    want = exp["match_unique"]
    halves = {key: ctr[1][key] + ctr[2][key] for key in ctr[0]}
    for what, i_, s_, c_ in (("whole", hi_[0], hs_[0], ctr[0]), ("halves", R.joined(hi_[1:]), R.joined(hs_[1:]) if scores else None, halves)):
        got = dict(info=i_, counters={key: int(c_[key]) for key in want["counters"]})
        if scores:
            got["score"] = s_.view(np.uint32)
        R.check("match_unique", got, what)
    # (the matcher's counters hold no launches: match_unique is not among the stages whose kernels are counted)
    info_h, score_h = hi_[0], hs_[0]
    want = exp["mapq"]
    R.note("mapq", m.mapq_stats(reset=True))
    qs, fin = [], []
    for k, (lo, hi) in enumerate(spans):
        q = m.mapq(P.records(hi_[k]), None if not scores else (P.records(hs_[k]) if P.device_records else hs_[k]), P.records(ha_[k]))
        qs.append(P.host(q, np.uint8))
        fin.append(_counters(m.mapq_stats(reset=True), want["finish"]))
    for what, a_, q, f in (("whole", ha_[0], qs[0], fin[0]), ("halves", R.joined(ha_[1:]), R.joined(qs[1:]), {key: fin[1][key] + fin[2][key] for key in fin[0]})):
        R.check("mapq", dict(acc=a_, mapq=q, finish=f), what)
    # 3: anchored gap placement over the same blocks, behind the matching: every block sees the final info words
    gaps = [None] * 3
    placed = [dict.fromkeys(gac.COUNTERS, 0) for _ in spans]             # the stage's counters of every run, summed over the blocks
    m.gap_anchor_stats(reset=True)
    resident = None
    for bi, (fid, first) in enumerate(blocks):
        g = dict(w.files)[fid]
        if resident != fid:
            m.set_text_symbols(fid, g.sym, g.frag_start)
            resident = fid
        m.build_index_block(first, per_block(cfg, g))
        for k, (lo, hi) in enumerate(spans):
            if bi == 0:
                out = P.output(hi - lo, rlib.GAP_PLACE_DTYPE)
                fresh = None if out is None else True
            else:
                out, fresh = gaps[k], False
            gaps[k] = m.match_gapped(mates[k], cfg.anchor_len, info=P.records(hi_[k]), out=out, fresh=fresh, max_anchors=cfg.max_anchors,
                                     host_records=P.mode == "mixed", **cfg.prm._asdict())
            st = m.gap_anchor_stats(reset=True)
            R.note("match_gapped", st)
            placed[k] = {key: placed[k][key] + int(st[key]) for key in gac.COUNTERS}
    hg = [P.host(x, rlib.GAP_PLACE_DTYPE) for x in gaps]
    for what, rec, c_ in (("whole", hg[0], placed[0]), ("halves", R.joined(hg[1:]), {key: placed[1][key] + placed[2][key] for key in gac.COUNTERS})):
        R.check("match_gapped", dict(gaps=rec, stats=c_), what)
    gaps_h = hg[0]
    # 4, 5: the read summaries and both markings
    want = exp["duplicates"]
    got = []
    for k, (lo, hi) in enumerate(spans):
        args, kw = P.flat(parts[k])
        out = np.zeros(hi - lo, dtype=rlib.READ_SUM_DTYPE) if P.mode == "mixed" else None
        got.append(P.host(m.read_summary(*args, min_qual=cfg.dedup_minq, out=out, **kw), rlib.READ_SUM_DTYPE))
    _same_or_diff(cfg, "duplicates", got[0], R.joined(got[1:]), "the summaries of the halves")
    sums = got[0]
    m.dup_stats(reset=True)
    dup1 = P.host(m.mark_duplicates(P.records(info_h), P.records(sums)), np.uint8)
    st1 = m.dup_stats(reset=True)
    dupg = P.host(m.mark_duplicates_gapped(P.records(info_h), P.records(gaps_h), P.records(sums)), np.uint8)
    stg = m.dup_stats()
    R.check("duplicates", dict(sums=sums, dup=dup1, stats=_counters(st1, want["stats"]), dup_gapped=dupg, stats_gapped=_counters(stg, want["stats_gapped"])))
    R.note("duplicates", st1)
    R.note("duplicates_gapped", stg)
    # 6: the mismatch lists of the ungapped placements (the main file is resident: the last one of the run)
    want = exp["mismatches"]
    got = []
    for k, (lo, hi) in enumerate(spans):
        if k < 2:
            m.mismatch_stats(reset=True)
        args, kw = P.flat(parts[k])
        lists, off = m.mismatches(*args, P.records(hi_[k]), **kw)
        got.append((P.host(lists, sk.MM_DTYPE), P.host(off, np.uint64)))
        if k != 1:
            st = m.mismatch_stats()
            lists, off = got[0] if k == 0 else R.lists_joined(got[1:])
            R.check("mismatches", dict(lists=lists, offsets=off, stats=_counters(st, want["stats"])), "whole" if k == 0 else "halves")
            R.note("mismatches", st)
    # 7, 8: the gapped consumers take the batch as both mates
    R.gapped_lists(mates_of, gaps_h)
    placed_info = dk.masked_info(info_h, dupg) if cfg.dedup else info_h
    placed_gaps = np.array(gaps_h, copy=True)
    if cfg.dedup:
        placed_gaps[dupg != 0] = m.new_gap_place(1)[0]

    def ungapped(add):
        def f(lo, hi):
            args, kw = P.flat(parts[spans.index((lo, hi))])
            add(*args, P.records(placed_info[lo:hi]), **kw)
        return f
    R.consumers(mates_of, placed_gaps, ungapped(m.pileup_add), ungapped(m.call_add))


def run(cfg: Config, ora, matcher_factory=make_matcher):
    """the chain of the configuration on the device, every stage compared with expected() before the next one runs -> {stage: launches}"""
    R = _Run(cfg, ora, matcher_factory)
    try:
        (_run_paired if cfg.kind == "paired" else _run_single)(R)
        R.finish()
    finally:
        R.m.close()                                                       # (a difference leaves no context open behind it)
    return R.launches


# ---- the floors: every configuration gives every stage work (checked with the checkers alone) ------------------------------------
def floors(cfg: Config, exp: dict) -> dict:
    """what a configuration gives the stages -> a dictionary of counts; assert_floors holds them against the conditions"""
    gap = exp["gap_rescue" if cfg.kind == "paired" else "match_gapped"]
    gaps = gap["gaps"]
    if cfg.kind == "paired":
        w = workload(cfg)
        ctr = {k: sum(gap["stats_%d" % fid][k] for fid, _ in w.files) for k in gc.COUNTERS}
    else:
        ctr = gap["stats"]
    state = gc.state_of(gaps["tag"])
    unique = state == gc.UNIQUE
    dup = exp["duplicates"]
    mm = exp["mismatches_pairs" if cfg.kind == "paired" else "mismatches"]
    first = exp["match_pairs_singles" if cfg.kind == "paired" else "match_unique"]
    q = exp["mapq"]["mapq"]
    return dict(placed=int(ctr["placed"]), unique=int(ctr["unique"]), gapped=int(ctr["gapped"]), skipped=int(ctr["skipped"]),
                deletions=int((unique & (gaps["gap"] > 0)).sum()), insertions=int((unique & (gaps["gap"] < 0)).sum()),
                nonunique=int((state == gc.NONUNIQUE).sum()), nomatch=int(ctr["eligible"] - ctr["placed"]),
                duplicates=int(dup["stats_gapped" if cfg.kind == "single" else "stats"]["duplicates"]),
                sites=int(exp["pileup"]["sites"].shape[0]), events=int(exp["indels"]["events"].shape[0]), mismatches=int(mm["lists"].shape[0]),
                snp_calls=int(exp["calls"]["calls"].shape[0]), indel_calls=int(exp["indels"]["indel_calls"].shape[0]),
                searched_changed=int((first["pairs"]["state"] != exp["_plain_pairs"]["state"]).sum()) if cfg.kind == "paired" else 0,
                mapq_below_60=int((q < 60).sum()))


def assert_floors(cfg: Config, f: dict):
    assert f["duplicates"] >= 1 and f["sites"] >= 1 and f["mismatches"] >= 1, (cfg, f)
    if not cfg.searched:                                                  # a read too short for the gap parameters: the stage skips it
        assert f["skipped"] > 0, (cfg, f)
        return
    assert f["placed"] >= 20 and f["unique"] >= 15 and f["gapped"] >= 10, (cfg, f)
    assert f["deletions"] >= 1 and f["insertions"] >= 1 and f["nonunique"] >= 1 and f["nomatch"] >= 1 and f["events"] >= 1, (cfg, f)
