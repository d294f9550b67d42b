"""Host-side mirror of the reference's interface for the read-matching path.

Names follow the reference: ``RealOptions`` (RealOptions.hpp:26-78, parser
RealOptions.cpp:122-466), ``UniqueMatcher.match`` / ``AllMatcher.match``
(matchUniqueImplementation.cpp:369-500, matchAllImplementation.cpp:261-355) --
here they take a whole decoded pattern block instead of one pattern, because the
device boundary sits at "for z in block: UM.match(...)" (SURVEY 3.1).

Everything below calls the C ABI of include/real_hip.h; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import lib as _lib
from .lib import (HIT_DTYPE, PAIR_DTYPE, PAIR_HIT_DTYPE, SINGLE_DTYPE, RealHipBatch, RealHipCounters, RealHipError, RealHipParams, _ptr)

NO_SCORE = np.float32(-np.finfo(np.float32).max)   # UniqueMatchInfo<true>() : score(-FLT_MAX), UniqueMatchInfo.hpp:191

# UniqueMatchInfoBase::MatchState, UniqueMatchInfo.hpp:71-78
NoMatch, Straight, Reverse, Gapped, NonUnique = 0, 1, 2, 3, 4


@dataclass
class RealOptions:
    """RealOptions.hpp:27-72; defaults :27-36."""
    textfilename: str = ""
    patternfilename: str = ""
    outputfilename: str = ""
    seedkmax: int = 2
    totalkmax: int = 5
    seedl: int = 32
    match_unique: bool = True
    fracmem: float = 0.75
    scores: bool = True
    qualityOffset: int = 0
    rewritepatterns: bool = True
    sort_threads: int = 2
    filter_level: int = 2
    similarity: float = 0.995
    err: float = 0.0
    trans: float = 0.71
    gc: float = 0.41
    gcmut_bias: float = 2.0
    gaps: bool = False
    pattern2filename: str = ""      # -p2: paired-end reads, mate 2 of every fragment (this build; no counterpart in the reference)
    insert_min: int = 0             # -insert_min / -insert_max: bounds of a concordant pair's outer distance
    insert_max: int = 1000
    mate_search: bool = False       # -mate_search: search every hit's window for a placement of the other mate the seeds missed
    mate_search_anchors: int = 0    # -mate_search_anchors: a mate with more hits than this contributes no anchors (0: no limit)
    pairs_all: bool = False         # -pairs_all: with -p2, print every concordant pair of a fragment instead of the unique one
    pairs_all_given: bool = False   # (the flag was on the command line: an error without -p2)
    unpairedfilename: str = ""      # -unpaired: with -p2, the file that receives the Unique mates of the fragments without a pair
    inserthistfilename: str = ""    # -insert_hist: with -p2, the file that receives the histogram of the Unique fragments' outer distances
    insert_auto: int = 0            # -insert_auto: with -p2, fragments the insert bounds are estimated from before the run (0: off)
    gappedfilename: str = ""        # -gapped: with -p2, the file that receives the mates placed with one insertion or deletion
    gap_max: int = 8                # -gap_max / -gap_flank / -gap_maxcost (-1: 4 * totalkmax + 6 + gap_max) / -gap_margin
    gap_flank: int = 8
    gap_maxcost: int = -1
    gap_margin: int = 0
    gappedsinglefilename: str = ""  # -gapped_single: without -p2, the file that receives the reads placed with one insertion or deletion
    gap_anchor: int = -1            # -gap_anchor (-1: max(seedl, 32)) / -gap_anchors
    gap_anchors: int = 32
    gpus: int = 1

    def normalise(self) -> "RealOptions":
        """The clamps of RealOptions.cpp:172-180, 434-453."""
        if self.totalkmax > 15:
            self.totalkmax = 15
        if self.seedl > 64:
            self.seedl = 64
        if self.seedl % 4:
            self.seedl -= self.seedl % 4
        if self.seedl < 4:
            raise ValueError("cannot handle seed length < 4")
        if self.seedkmax > 2:
            self.seedkmax = 2
        if self.gappedfilename:         # the loud errors of `real -gapped`
            if not self.pattern2filename:
                raise ValueError("-gapped needs -p2 (paired-end reads)")
            if self.pairs_all:
                raise ValueError("-gapped cannot be combined with -pairs_all 1")
            if self.gappedfilename in (self.outputfilename, self.unpairedfilename, self.inserthistfilename):
                raise ValueError("-gapped names the same file as another output")
            if not 1 <= self.gap_max <= _lib.GAP_MAX:
                raise ValueError("-gap_max must be in 1..%d" % _lib.GAP_MAX)
            if self.gap_flank < 1:
                raise ValueError("-gap_flank must be at least 1")
            if self.gap_maxcost < 0:
                self.gap_maxcost = 4 * self.totalkmax + 6 + self.gap_max
            if self.insert_max > _lib.REAL_HIP_MATE_SEARCH_MAX_INSERT:
                raise ValueError("-gapped takes an -insert_max of at most %d" % _lib.REAL_HIP_MATE_SEARCH_MAX_INSERT)
        if self.gappedsinglefilename:   # the loud errors of `real -gapped_single`
            if self.pattern2filename:
                raise ValueError("-gapped_single places single reads: with -p2 the flag is -gapped")
            if not self.match_unique:
                raise ValueError("-gapped_single cannot be combined with -u 0")
            if self.gappedsinglefilename == self.outputfilename:
                raise ValueError("-gapped_single names the same file as -o")
            if not 1 <= self.gap_max <= _lib.GAP_MAX:
                raise ValueError("-gap_max must be in 1..%d" % _lib.GAP_MAX)
            if self.gap_flank < 1:
                raise ValueError("-gap_flank must be at least 1")
            if self.gap_maxcost < 0:
                self.gap_maxcost = 4 * self.totalkmax + 6 + self.gap_max
            if self.gap_anchor < 0:
                self.gap_anchor = max(self.seedl, 32)
            if not 1 <= self.gap_anchor <= _lib.REAL_HIP_MAX_PATL:
                raise ValueError("-gap_anchor must be in 1..%d" % _lib.REAL_HIP_MAX_PATL)
            if not 1 <= self.gap_anchors <= _lib.GAP_ANCHORS_MAX:
                raise ValueError("-gap_anchors must be in 1..%d" % _lib.GAP_ANCHORS_MAX)
        if self.pattern2filename:       # the loud errors of `real -p2`
            if not self.match_unique:
                raise ValueError("-p2 (paired-end reads) cannot be combined with -u 0 (every concordant pair: -pairs_all 1)")
            if self.gpus > 1:
                raise ValueError("-p2 (paired-end reads) cannot be combined with -gpus > 1")
            if self.insert_min > self.insert_max:
                raise ValueError("-insert_min is larger than -insert_max")
            if self.mate_search and self.insert_max > _lib.REAL_HIP_MATE_SEARCH_MAX_INSERT:
                raise ValueError("-mate_search 1 takes an -insert_max of at most %d" % _lib.REAL_HIP_MATE_SEARCH_MAX_INSERT)
            if self.pairs_all and self.mate_search:
                raise ValueError("-pairs_all 1 lists pairs of two seed hits: it cannot be combined with -mate_search 1")
            if self.unpairedfilename and self.pairs_all:
                raise ValueError("-unpaired lists the mates of the fragments without a pair: it cannot be combined with -pairs_all 1")
            if self.unpairedfilename and self.unpairedfilename == self.outputfilename:
                raise ValueError("-unpaired names the same file as -o")
            if self.inserthistfilename or self.insert_auto:
                if self.pairs_all:
                    raise ValueError("-insert_hist / -insert_auto cannot be combined with -pairs_all 1")
                if self.insert_max > _lib.REAL_HIP_INSERT_HIST_MAX_BINS - 2:
                    raise ValueError("-insert_hist / -insert_auto take an -insert_max of at most %d" % (_lib.REAL_HIP_INSERT_HIST_MAX_BINS - 2))
                if self.inserthistfilename and self.inserthistfilename in (self.outputfilename, self.unpairedfilename):
                    raise ValueError("-insert_hist names the same file as -o or -unpaired")
        elif self.inserthistfilename or self.insert_auto:
            raise ValueError("-insert_hist / -insert_auto need -p2 (paired-end reads)")
        elif self.unpairedfilename:
            raise ValueError("-unpaired needs -p2 (paired-end reads)")
        elif self.mate_search or self.mate_search_anchors:
            raise ValueError("-mate_search / -mate_search_anchors need -p2 (paired-end reads)")
        elif self.pairs_all or self.pairs_all_given:
            raise ValueError("-pairs_all needs -p2 (paired-end reads)")
        if self.mate_search_anchors < 0:
            raise ValueError("-mate_search_anchors must not be negative")
        return self

    @property
    def filter_mult(self) -> float:
        """RealOptions.cpp:455-463."""
        mult = {1: 0.5, 2: 1.0, 3: 2.0, 4: 3.0}.get(self.filter_level, 0.0) * self.totalkmax
        return mult / 70.0

    def getFilterValue(self, patl: int) -> float:
        """RealOptions.hpp:74-77."""
        return self.filter_mult * patl

    @classmethod
    def parse(cls, argv: Sequence[str]) -> "RealOptions":
        """The hand-rolled argv loop of RealOptions.cpp:140-396 (unknown arguments are ignored)."""
        o = cls()
        i = 0
        table = {"-t": ("textfilename", str), "-p": ("patternfilename", str), "-o": ("outputfilename", str),
                 "-s": ("seedkmax", int), "-e": ("totalkmax", int), "-l": ("seedl", int),
                 "-u": ("match_unique", lambda v: bool(int(v))), "-f": ("fracmem", float), "-m": ("fracmem", float),
                 "-q": ("scores", lambda v: bool(int(v))), "-Q": ("qualityOffset", int),
                 "-R": ("rewritepatterns", lambda v: bool(int(v))), "-T": ("sort_threads", int),
                 "-g": ("gaps", lambda v: bool(int(v))), "-similarity": ("similarity", float), "-err": ("err", float),
                 "-trans": ("trans", float), "-gc": ("gc", float), "-gcmut_bias": ("gcmut_bias", float),
                 "-filter_level": ("filter_level", int), "-p2": ("pattern2filename", str), "-insert_min": ("insert_min", int),
                 "-insert_max": ("insert_max", int), "-gpus": ("gpus", int),
                 "-mate_search": ("mate_search", lambda v: bool(int(v))), "-mate_search_anchors": ("mate_search_anchors", int),
                 "-pairs_all": ("pairs_all", lambda v: bool(int(v))), "-unpaired": ("unpairedfilename", str),
                 "-insert_hist": ("inserthistfilename", str), "-insert_auto": ("insert_auto", int),
                 "-gapped": ("gappedfilename", str), "-gap_max": ("gap_max", int), "-gap_flank": ("gap_flank", int),
                 "-gap_maxcost": ("gap_maxcost", int), "-gap_margin": ("gap_margin", int),
                 "-gapped_single": ("gappedsinglefilename", str), "-gap_anchor": ("gap_anchor", int), "-gap_anchors": ("gap_anchors", int)}
        argv = list(argv)
        while i < len(argv):
            a = argv[i]
            if a in table:
                if i + 1 >= len(argv):
                    raise ValueError("Parameter for argument %s is missing." % a)
                name, conv = table[a]
                setattr(o, name, conv(argv[i + 1]))
                if a == "-pairs_all":
                    o.pairs_all_given = True
                i += 2
            else:
                i += 1
        return o.normalise()


def new_unique_info(n: int, scores: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """AutoArray<UniqueMatchInfo<scores>> uniqueinfo(numpat), matchUniqueImplementation.cpp:1094-1097."""
    info = np.zeros(n, dtype=np.uint64)
    score = np.full(n, NO_SCORE, dtype=np.float32) if scores else None
    return info, score


def new_pair_info(n: int) -> np.ndarray:
    """the records of n fragments before the first genome file: no pair, best = second = -inf (real_hip_pair)"""
    rec = np.zeros(n, dtype=PAIR_DTYPE)
    rec["best"] = -np.inf
    rec["second"] = -np.inf
    return rec


def new_single_info(n: int) -> np.ndarray:
    """the records of n reads before the first genome file: empty (state NoMatch, score 0, second -inf; real_hip_single)"""
    rec = np.zeros(n, dtype=SINGLE_DTYPE)
    rec["second"] = -np.inf
    return rec


def new_gap_place(n: int) -> np.ndarray:
    """the gap records of n fragments before the first genome file: NoMatch (real_hip_gap_place)"""
    rec = np.zeros(n, dtype=_lib.GAP_PLACE_DTYPE)
    rec["second"] = _lib.GAP_NONE
    return rec


def new_mapq_acc(n: int) -> np.ndarray:
    """the accumulators of n reads (fragments) before the first index block: empty (real_hip_mapq_acc)"""
    rec = np.zeros(n, dtype=_lib.MAPQ_ACC_DTYPE)
    rec["level"] = _lib.MAPQ_EMPTY_LEVEL
    return rec


def unpack_info(info: np.ndarray):
    """UniqueMatchInfo.hpp:29-39 -> state, fragment, errors, fileid, position."""
    rec = np.asarray(info, dtype=np.uint64)
    state = np.minimum(rec >> np.uint64(61), np.uint64(4)).astype(np.int64)
    frag = ((rec >> np.uint64(45)) & np.uint64(0xffff)).astype(np.int64)
    err = ((rec >> np.uint64(41)) & np.uint64(15)).astype(np.int64)
    fid = ((rec >> np.uint64(35)) & np.uint64(63)).astype(np.int64)
    pos = (rec & np.uint64((1 << 35) - 1)).astype(np.int64)
    return state, frag, err, fid, pos


def _start_or_fold(records, fresh: Optional[bool], on_device: bool, new, what: str = "records"):
    """In/out records across genome files -> (records, fresh).  None starts them: new() on the host (device inputs need the
    caller's tensor), and the call is fresh; given records are folded into unless fresh says they are output only."""
    if fresh is None:
        fresh = records is None
    if records is None:
        if on_device:
            raise ValueError("device inputs need a device tensor for the %s" % what)
        records = new()
    return records, bool(fresh)


def _held_lists(mates, differ: str, batch: Optional[RealHipBatch] = None):
    """Hit lists the caller holds, one (hits, offsets, lengths or None) per mate -> (on_device, n, the lists as the library
    reads them): lib.HIT_DTYPE / uint64 / uint32 unless they are device tensors, all describing n reads, else
    ValueError(differ).  Where they lie and n are the batch's when they come with one, else the first offsets'."""
    on_device = bool(batch.on_device if batch is not None else getattr(mates[0][1], "is_cuda", False))
    n = None if batch is None else int(batch.n_reads)
    out = []
    for hits, off, lens in mates:
        if not on_device:
            hits, off = np.ascontiguousarray(hits, dtype=HIT_DTYPE), np.ascontiguousarray(off, dtype=np.uint64)
            lens = None if lens is None else np.ascontiguousarray(lens, dtype=np.uint32)
        if n is None:
            n = int(off.shape[0]) - 1
        if int(off.shape[0]) - 1 != n or (lens is not None and int(lens.shape[0]) != n):
            raise ValueError(differ)
        out.append((hits, off, lens))
    return on_device, n, out


class HipMatcher:
    """One context on one MI355X: resident text + index block + matching calls."""

    def __init__(self, opts: RealOptions, device: int = 0, prefix_bits: int = 0, LL: Optional[np.ndarray] = None,
                 table_kind: int = 0):
        self.opts = opts
        self._L = _lib.load()
        self._pinned = []                  # what host_alloc handed out: freed with the matcher
        # table_kind is a request: 0 auto, 1 bucket starts only, 2 directory entries, 3 bucket rows (real_hip.h)
        p = _lib.sized(RealHipParams, seedl=opts.seedl, seedkmax=opts.seedkmax, totalkmax=opts.totalkmax, scores=int(bool(opts.scores)),
                       prefix_bits=prefix_bits, table_kind=table_kind, device=device, filter_mult=opts.filter_mult)
        if LL is None:
            LL = _lib.scoring_table(opts.similarity, opts.gc, opts.trans, opts.err, opts.gcmut_bias)
        self.LL = np.ascontiguousarray(LL, dtype=np.float64)
        for i in range(1024):
            p.LL[i] = float(self.LL[i])
        h = C.c_void_p()
        rc = self._L.real_hip_create(C.byref(h), C.byref(p))
        if rc != 0:
            raise RealHipError(rc, self._L.real_hip_strerror(rc).decode() +
                               " (real_hip_create: is an MI355X visible? there is no CPU fallback)")
        self._h = h
        self.device = device
        self.n_entries = 0
        self.prefix_bits = 0

    # -- lifetime --
    def close(self):
        if getattr(self, "_h", None):
            self._L.real_hip_destroy(self._h)
            self._h = None
        for p in getattr(self, "_pinned", []):
            self._L.real_hip_host_free(p)
        self._pinned = []

    def __del__(self):
        self.close()

    def _check(self, rc: int):
        if rc != 0:
            raise RealHipError(rc, self._L.real_hip_last_error(self._h).decode() or self._L.real_hip_strerror(rc).decode())

    def set_match_params(self, seedkmax: Optional[int] = None, totalkmax: Optional[int] = None, scores: Optional[bool] = None,
                         filter_level: Optional[int] = None):
        """-s / -e / -q / -filter_level for the calls that follow; the resident text and index stay (they depend on -l only)."""
        o = self.opts
        if seedkmax is not None: o.seedkmax = seedkmax
        if totalkmax is not None: o.totalkmax = totalkmax
        if scores is not None: o.scores = bool(scores)
        if filter_level is not None: o.filter_level = filter_level
        o.normalise()
        self._check(self._L.real_hip_set_match_params(self._h, o.seedkmax, o.totalkmax, int(bool(o.scores)), o.filter_mult))

    # -- text --
    def set_text(self, fileid: int, text2bit: np.ndarray, wildbits: np.ndarray, n_bases: int, frag_start: np.ndarray):
        t = np.ascontiguousarray(text2bit, dtype=np.uint64)
        w = np.ascontiguousarray(wildbits, dtype=np.uint64)
        f = np.ascontiguousarray(frag_start, dtype=np.uint64)
        self._check(self._L.real_hip_set_text(self._h, fileid, t.ctypes.data, w.ctypes.data, n_bases, f.ctypes.data, f.shape[0] - 1))

    def set_text_symbols(self, fileid: int, sym, frag_start: np.ndarray, n_bases: Optional[int] = None):
        """sym: numpy uint8 (host) or a torch uint8 tensor (host or device)."""
        f = np.ascontiguousarray(frag_start, dtype=np.uint64)
        on_device = bool(getattr(sym, "is_cuda", False))
        self.sync_inputs(sym)
        if isinstance(sym, np.ndarray):
            sym = np.ascontiguousarray(sym, dtype=np.uint8)
        n = int(n_bases if n_bases is not None else sym.shape[0])
        self._check(self._L.real_hip_set_text_symbols(self._h, fileid, _ptr(sym), n, int(on_device), f.ctypes.data, f.shape[0] - 1))

    # -- index --
    def set_index_block(self, sign: Sequence[np.ndarray], pos: Sequence[np.ndarray]):
        """Host-built sorted lists (ListSetBlockReader::readNextBlock, ListSetBlockReader.hpp:24-52)."""
        sdt = np.uint32 if self.opts.seedl <= 32 else np.uint64
        sg = [np.ascontiguousarray(s, dtype=sdt) for s in sign]
        ps = [np.ascontiguousarray(p, dtype=np.uint32) for p in pos]
        n = int(sg[0].shape[0])
        sa = (C.c_void_p * 6)(*[s.ctypes.data for s in sg])
        pa = (C.c_void_p * 6)(*[p.ctypes.data for p in ps])
        self._check(self._L.real_hip_set_index_block(self._h, n, sa, pa))
        self._refresh_index_info()

    def build_index_block(self, first_window: int = 0, max_entries: int = (1 << 62)) -> Tuple[int, bool]:
        n = C.c_uint64(0)
        nxt = C.c_int(0)
        self._check(self._L.real_hip_build_index_block(self._h, first_window, max_entries, C.byref(n), C.byref(nxt)))
        self._refresh_index_info()
        return int(n.value), bool(nxt.value)

    def _stats(self, struct, entry, reset: bool) -> dict:
        """one read of a statistics struct of the ABI: every field the struct names, times (*_ms) as float, counts as int"""
        st = _lib.sized(struct)
        self._check(entry(self._h, C.byref(st), int(reset)))
        return {k: (float if k.endswith("_ms") else int)(getattr(st, k)) for k in _lib.stats_fields(struct)}

    def index_build_stats(self, reset: bool = False) -> dict:
        """where the wall time of this context's index builds went (real_hip_index_build_stats)"""
        return self._stats(_lib.RealHipBuildStats, self._L.real_hip_index_build_stats, reset)

    def _refresh_index_info(self):
        n = C.c_uint64(0)
        pb = C.c_uint32(0)
        self._check(self._L.real_hip_index_info(self._h, C.byref(n), C.byref(pb)))
        self.n_entries, self.prefix_bits = int(n.value), int(pb.value)
        tk = C.c_uint32(0)
        self._check(self._L.real_hip_index_table_kind(self._h, C.byref(tk)))
        self.table_kind = int(tk.value)   # the layout built: lib.LAYOUT_STARTS .. lib.LAYOUT_ROWS

    def index_download(self, k: int, want_buckets: bool = True):
        """device layout of list k: entries (n x {fingerprint, pos}) and bucket starts."""
        ent = np.zeros((self.n_entries, 2), dtype=np.uint32)
        bkt = np.zeros((1 << self.prefix_bits) + 1, dtype=np.uint32) if want_buckets else None
        self._check(self._L.real_hip_index_download(self._h, k, ent.ctypes.data, _ptr(bkt)))
        return ent, bkt

    def index_export(self, k: int):
        """list k in the reference's form: (sign[n], pos[n]) of the sorted Mask entries."""
        sdt = np.uint32 if self.opts.seedl <= 32 else np.uint64
        sign = np.zeros(self.n_entries, dtype=sdt)
        pos = np.zeros(self.n_entries, dtype=np.uint32)
        self._check(self._L.real_hip_index_export(self._h, k, sign.ctypes.data, pos.ctypes.data))
        return sign, pos

    # -- batches --
    @staticmethod
    def sync_inputs(*arrays):
        """The library runs on the context's own stream and does not know the caller's: device arrays handed over
        (inputs AND in/out records) must be complete before the call (include/real_hip.h, "Streams").  For torch
        tensors that means the producing stream has to drain -- done here, once per device."""
        seen = set()
        for a in arrays:
            if a is not None and getattr(a, "is_cuda", False) and a.device not in seen:
                import torch
                torch.cuda.current_stream(a.device).synchronize()
                seen.add(a.device)

    @staticmethod
    def _batch(bases, qual, offsets, patl: int, n_reads: Optional[int], max_patl: int = 0) -> RealHipBatch:
        """the struct alone, over arrays as they stand: where they lie, how many reads, the addresses"""
        if offsets is not None and not isinstance(offsets, int):
            n_reads = int(offsets.shape[0]) - 1
        elif n_reads is None:
            n_reads = bases.shape[0] // patl
        return _lib.sized(RealHipBatch, on_device=int(bool(getattr(bases, "is_cuda", False))), n_reads=int(n_reads), bases=_ptr(bases),
                          qual=_ptr(qual), offsets=_ptr(offsets), patl=int(patl), max_patl=int(max_patl))

    @staticmethod
    def _read_batch(bases, qual, offsets=None, *, patl: int = 0, n_reads: Optional[int] = None, max_patl: int = 0,
                    packed: bool = False, nflags=None, fresh: bool = False, host_records: bool = False,
                    on_device: Optional[int] = None, copy: bool = True) -> RealHipBatch:
        """The batch of every entry point.  Host numpy arrays are made contiguous uint8 / uint8 / uint64 (copy=False: the
        arrays must stay the caller's, one that is not contiguous is refused); n_reads comes from the offsets, else from the
        argument, else from patl.  on_device is 0 for host arrays, 1 for device tensors, 2 for device tensors whose records live
        on the host (host_records), or what the caller says of raw addresses.  The struct keeps alive what it points to, and
        the arrays are complete when this returns (sync_inputs)."""
        if isinstance(bases, np.ndarray):
            given = (bases, qual, offsets)
            if copy:
                bases, qual, offsets = (None if a is None else np.ascontiguousarray(a, dtype=t)
                                        for a, t in zip(given, (np.uint8, np.uint8, np.uint64)))
            elif not all(a is None or a.flags.c_contiguous for a in given):
                raise ValueError("the arrays of a submitted batch are not copied: they must be contiguous")
        if packed and offsets is None and n_reads is None:
            raise ValueError("a packed batch of uniform length needs n_reads")
        b = HipMatcher._batch(bases, qual, offsets, patl, n_reads, max_patl)
        if on_device is not None:
            b.on_device = on_device
        elif b.on_device and host_records:
            b.on_device = 2
        b.packed, b.fresh, b.nflags = int(bool(packed)), int(bool(fresh)), _ptr(nflags)
        b._keep = (bases, qual, offsets, nflags)
        HipMatcher.sync_inputs(bases, qual, offsets, nflags)
        return b

    def _mate_batch(self, mate, **kw) -> RealHipBatch:
        """mate: a synth.ReadBatch-like object (bases, qual, offsets) or a tuple (bases, qual, offsets)"""
        bases, qual, offsets = (mate.bases, mate.qual, mate.offsets) if hasattr(mate, "bases") else mate
        return self._read_batch(bases, qual, offsets, **kw)

    def _grown(self, call, room, cap: int, offsets=None):
        """The overflow protocol of every list the library returns: call(out, cap, n_out, offsets) once with room(cap) records;
        on REAL_HIP_E_OVERFLOW once more with exactly the count it reported -> the records written.  The count is exact, so a
        second overflow is a fault and surfaces as RealHipError."""
        n = C.c_uint64(0)

        def attempt(cap):
            out = room(cap)
            self.sync_inputs(out, offsets)
            return out, call(_ptr(out), cap, C.byref(n), _ptr(offsets))
        out, rc = attempt(int(cap))
        if rc == _lib.REAL_HIP_E_OVERFLOW:
            out, rc = attempt(int(n.value))
        self._check(rc)
        return out[:int(n.value)]

    def _host_list(self, entry, dtype, cap: int) -> np.ndarray:
        """a list the context holds (sites, evidence, calls) as numpy records of `dtype`"""
        return self._grown(lambda o, c, no, _: entry(self._h, o, c, no, 0), lambda c: np.zeros(c, dtype=dtype), cap)

    def match_unique(self, bases, qual, offsets=None, patl: int = 0, info=None, score=None,
                     n_reads: Optional[int] = None, max_patl: int = 0, packed: bool = False, nflags=None,
                     fresh: bool = False):
        """UniqueMatcher::match over a pattern block, folding into info/score in place.
        Host numpy arrays or device torch tensors (all of one kind).  fresh: info / score are outputs only, every
        record starts as uniqueinfo(numpat) does (the first genome block of a run)."""
        b = self._read_batch(bases, qual, offsets, patl=patl, n_reads=n_reads, max_patl=max_patl, packed=packed, nflags=nflags, fresh=fresh)
        return self._match_unique(b, info, score)

    def _match_unique(self, b: RealHipBatch, info, score):
        if info is None:
            info, score = new_unique_info(int(b.n_reads), self.opts.scores)
        self.sync_inputs(info, score)
        self._check(self._L.real_hip_match_unique(self._h, C.byref(b), _ptr(info), _ptr(score)))
        return info, score

    def match_all(self, bases, qual, offsets=None, patl: int = 0, n_reads: Optional[int] = None, cap: int = 0):
        """AllMatcher::match + unifyMatches over a host pattern block -> (hits, hit_offsets)."""
        b = self._read_batch(np.asarray(bases), qual, offsets, patl=patl, n_reads=n_reads)
        n = int(b.n_reads)
        hoff = np.zeros(n + 1, dtype=np.uint64)
        hits = self._grown(lambda o, c, no, po: self._L.real_hip_match_all(self._h, C.byref(b), o, c, no, po),
                           lambda c: np.zeros(c, dtype=HIT_DTYPE), cap or max(1024, 4 * n), hoff)
        return hits, hoff

    # -- pipelined host batches (submit / wait over two slots) --
    def host_alloc(self, shape, dtype) -> np.ndarray:
        """a numpy array over pinned host memory (real_hip_host_alloc): batches handed over from it cross PCIe by DMA
        without a staging copy, which is what makes submit asynchronous.  Freed with the matcher."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape))
        p = self._L.real_hip_host_alloc(max(1, n * dt.itemsize))
        if not p:
            raise RealHipError(_lib.REAL_HIP_E_NOMEM, "real_hip_host_alloc")
        self._pinned.append(p)
        buf = (C.c_uint8 * (n * dt.itemsize)).from_address(p)
        return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)

    def submit_unique(self, slot: int, bases, qual, info, score, patl: int = 0, offsets=None, n_reads: Optional[int] = None,
                      packed: bool = False, nflags=None, fresh: bool = False):
        """real_hip_match_unique_submit: queue upload, kernels and download of one host batch; returns at once.  The
        arrays must stay alive and untouched until wait(slot)."""
        b = self._read_batch(bases, qual, offsets, patl=patl, n_reads=n_reads, packed=packed, nflags=nflags, on_device=0, copy=False)
        self._check(self._L.real_hip_match_unique_submit(self._h, C.byref(b), _ptr(info), _ptr(score), slot, int(bool(fresh))))

    def wait(self, slot: int):
        self._check(self._L.real_hip_wait(self._h, slot))

    # -- multi-GPU: the C ABI's own RCCL gather (one process per GPU; torch.distributed is the other way, real_amd.distributed) --
    @staticmethod
    def comm_id() -> bytes:
        """rank 0: the 128 bytes every rank hands to comm_init (broadcast them by the launcher's own means)"""
        buf = (C.c_uint8 * 128)()
        rc = _lib.load().real_hip_comm_id(buf)
        if rc != 0:
            raise RealHipError(rc, "real_hip_comm_id (librccl could not be loaded?)")
        return bytes(buf)

    def comm_init(self, comm_id: bytes, rank: int, n_ranks: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(comm_id)
        self._check(self._L.real_hip_comm_init(self._h, buf, rank, n_ranks))

    def gather_records(self, root: int, info, score, info_all=None, score_all=None) -> int:
        """device tensors; returns the number of records on the root (real_hip_gather_records)"""
        self.sync_inputs(info, score, info_all, score_all)
        n_all = C.c_uint64(0)
        cap = int(info_all.shape[0]) if info_all is not None else 0
        self._check(self._L.real_hip_gather_records(self._h, root, _ptr(info), _ptr(score), int(info.shape[0]), _ptr(info_all), _ptr(score_all), cap, C.byref(n_all)))
        return int(n_all.value)

    def gather_hits(self, root: int, hits, hit_offsets, n_hits: int, hits_all=None, offsets_all=None):
        """device tensors: hits [n, 4] int32 (real_hip_hit records), hit_offsets [n_local + 1] int64; returns (reads, hits) on the root"""
        self.sync_inputs(hits, hit_offsets, hits_all, offsets_all)
        nr, nh = C.c_uint64(0), C.c_uint64(0)
        cap_h = int(hits_all.shape[0]) if hits_all is not None else 0
        cap_r = int(offsets_all.shape[0]) - 1 if offsets_all is not None else 0
        self._check(self._L.real_hip_gather_hits(self._h, root, _ptr(hits), _ptr(hit_offsets), int(hit_offsets.shape[0]) - 1, int(n_hits), _ptr(hits_all), cap_h,
                                                 _ptr(offsets_all), cap_r, C.byref(nr), C.byref(nh)))
        return int(nr.value), int(nh.value)

    # -- read ingestion on the device --
    def parse_reads(self, text, fastq: bool, quality_offset: int = 33):
        """FASTA / FASTQ text (bytes, numpy uint8 or a device torch tensor) -> RealHipParsed: device arrays owned by the
        context, valid until the next parse.  Raises RealHipError(E_UNSUPPORTED) for text that is not in
        one-line-per-field form (FastQReader.hpp:130-180 accepts more; the host reader handles that)."""
        on_dev = bool(getattr(text, "is_cuda", False))
        if not on_dev and not isinstance(text, np.ndarray):
            text = np.frombuffer(text, dtype=np.uint8)
        n = int(text.numel()) if on_dev else int(text.shape[0])
        self.sync_inputs(text)
        out = _lib.RealHipParsed()
        self._check(self._L.real_hip_parse_reads(self._h, _ptr(text), n, int(on_dev), int(bool(fastq)), int(quality_offset), C.byref(out)))
        return out

    def match_unique_parsed(self, parsed, info=None, score=None):
        """UniqueMatcher::match over the reads of a parse_reads() result (read arrays on the device, records on the host)."""
        b = self._read_batch(parsed.bases, parsed.qual, parsed.offsets, n_reads=parsed.n_reads, max_patl=parsed.max_patl, on_device=2)
        return self._match_unique(b, info, score)

    def download(self, dev_ptr, count: int, dtype):
        """copy `count` items of a device array the library returned to the host (tests, id strings)"""
        out = np.zeros(count, dtype=dtype)
        if count:
            self._check(self._L.real_hip_download(self._h, C.c_void_p(int(dev_ptr)), out.ctypes.data, out.nbytes))
        return out

    # -- pileup: depth and mismatch base counts per position of the resident text (include/real_hip.h, "pileup") --
    def pileup_begin(self, min_qual: int = 0):
        """real_hip_pileup_begin: accumulators for the resident text, zeroed; a second begin starts again"""
        p = _lib.sized(_lib.RealHipPileupParams, min_qual=int(min_qual))
        self._check(self._L.real_hip_pileup_begin(self._h, C.byref(p)))

    # -- the stages behind the matching (pileup, calls, mismatch lists): reads and their final records --
    def _placed(self, bases, qual, info, **kw):
        """a batch and its records for a stage -> (batch, info): numpy records are made contiguous (with device reads they stay
        on the host: on_device = 2), and there is one record per read"""
        host = isinstance(info, np.ndarray)
        if host:
            info = np.ascontiguousarray(info, dtype=np.uint64)
        b = self._read_batch(bases, qual, host_records=host, **kw)
        if int(info.shape[0]) != int(b.n_reads):
            raise ValueError("one record per read")
        self.sync_inputs(info)
        return b, info

    def _placed_pairs(self, mate1, mate2, pairs, singles1=None, singles2=None):
        """both mates' batches and the fragments' records for a stage -> (batch 1, batch 2, pairs, singles1, singles2)"""
        host = isinstance(pairs, np.ndarray)
        if host:
            pairs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
            singles1, singles2 = (None if s is None else np.ascontiguousarray(s, dtype=SINGLE_DTYPE) for s in (singles1, singles2))
        b1, b2 = self._mate_batch(mate1, host_records=host), self._mate_batch(mate2, host_records=host)
        self.sync_inputs(pairs, singles1, singles2)
        return b1, b2, pairs, singles1, singles2

    def pileup_add(self, bases, qual, info, offsets=None, patl: int = 0, n_reads: Optional[int] = None, max_patl: int = 0,
                   packed: bool = False, nflags=None):
        """real_hip_pileup_add: the placements of the records `info` (what match_unique returned for this batch).  Host
        numpy arrays, device torch tensors, or device reads with numpy records (on_device = 2)."""
        b, info = self._placed(bases, qual, info, offsets=offsets, patl=patl, n_reads=n_reads, max_patl=max_patl, packed=packed, nflags=nflags)
        self._check(self._L.real_hip_pileup_add(self._h, C.byref(b), _ptr(info)))

    def pileup_add_pairs(self, mate1, mate2, pairs):
        """real_hip_pileup_add_pairs: both mates of every Unique record of `pairs` (what match_pairs returned); mates as
        (bases, qual, offsets) tuples or ReadBatch-like objects, all host arrays or all device tensors"""
        b1, b2, pairs, _, _ = self._placed_pairs(mate1, mate2, pairs)
        self._check(self._L.real_hip_pileup_add_pairs(self._h, C.byref(b1), C.byref(b2), _ptr(pairs)))

    def pileup_finish(self) -> int:
        """real_hip_pileup_finish: scans the depth and compacts the sites; returns the number of sites"""
        n = C.c_uint64(0)
        self._check(self._L.real_hip_pileup_finish(self._h, C.byref(n)))
        return int(n.value)

    def pileup_depth(self, first: int, count: int, out=None) -> np.ndarray:
        """depth[first .. first + count) as numpy uint32 (out: a device torch tensor of count 32-bit words instead)"""
        on_device = bool(getattr(out, "is_cuda", False))
        if out is None:
            out = np.zeros(int(count), dtype=np.uint32)
        self.sync_inputs(out)
        self._check(self._L.real_hip_pileup_depth(self._h, int(first), int(count), _ptr(out), int(on_device)))
        return out

    def pileup_sites(self, cap: int = 1024) -> np.ndarray:
        """the site list as lib.PILEUP_SITE_DTYPE, ascending position; the buffer grows once to the size the library reports"""
        return self._host_list(self._L.real_hip_pileup_sites, _lib.PILEUP_SITE_DTYPE, cap)

    def pileup_end(self):
        self._check(self._L.real_hip_pileup_end(self._h))

    def pileup_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipPileupStats, self._L.real_hip_pileup_stats_get, reset)

    # -- variant calls: genotypes of the finished pileup's sites (include/real_hip.h, "variant calls") --
    def call_begin(self):
        """real_hip_call_begin: site bitmap, rank array and zeroed evidence of the finished pileup; a second begin starts again"""
        self._check(self._L.real_hip_call_begin(self._h))

    def call_add(self, bases, qual, info, offsets=None, patl: int = 0, n_reads: Optional[int] = None, max_patl: int = 0,
                 packed: bool = False, nflags=None):
        """real_hip_call_add: the evidence of the placements of `info`; the arguments are pileup_add's"""
        b, info = self._placed(bases, qual, info, offsets=offsets, patl=patl, n_reads=n_reads, max_patl=max_patl, packed=packed, nflags=nflags)
        self._check(self._L.real_hip_call_add(self._h, C.byref(b), _ptr(info)))

    def call_add_pairs(self, mate1, mate2, pairs):
        """real_hip_call_add_pairs: both mates of every Unique record of `pairs`; the arguments are pileup_add_pairs'"""
        b1, b2, pairs, _, _ = self._placed_pairs(mate1, mate2, pairs)
        self._check(self._L.real_hip_call_add_pairs(self._h, C.byref(b1), C.byref(b2), _ptr(pairs)))

    def call_finish(self, min_call_qual: int = 20, min_depth: int = 4) -> int:
        """real_hip_call_finish: the genotypes and the compacted call list; returns the number of calls.  May be called again
        with other thresholds"""
        p = _lib.sized(_lib.RealHipCallParams, min_call_qual=int(min_call_qual), min_depth=int(min_depth))
        n = C.c_uint64(0)
        self._check(self._L.real_hip_call_finish(self._h, C.byref(p), C.byref(n)))
        return int(n.value)

    def call_evidence(self, cap: int = 1024) -> np.ndarray:
        """the evidence table as lib.CALL_EVIDENCE_DTYPE, record s for site s of pileup_sites(); the buffer grows once"""
        return self._host_list(self._L.real_hip_call_evidence, _lib.CALL_EVIDENCE_DTYPE, cap)

    def call_variants(self, cap: int = 1024) -> np.ndarray:
        """the call list as lib.CALL_DTYPE, ascending position; the buffer grows once to the size the library reports"""
        return self._host_list(self._L.real_hip_call_variants, _lib.CALL_DTYPE, cap)

    def call_end(self):
        self._check(self._L.real_hip_call_end(self._h))

    def call_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipCallStats, self._L.real_hip_call_stats_get, reset)

    # -- mismatch lists: where each placed read differs from the resident text (include/real_hip.h, "mismatch lists") --
    def _mismatch_call(self, call, lists: int, on_device: bool, cap: int):
        """one list call with its outputs: host numpy arrays, or device tensors when the records are; the buffer grows once to
        the size the library reports -> (lists as lib.MISMATCH_DTYPE, offsets)"""
        if on_device:
            import torch
            off = torch.zeros(lists + 1, dtype=torch.int64, device="cuda")
            room = lambda c: torch.zeros(max(c, 1), dtype=torch.int32, device="cuda")       # noqa: E731
        else:
            off = np.zeros(lists + 1, dtype=np.uint64)
            room = lambda c: np.zeros(c, dtype=_lib.MISMATCH_DTYPE)                         # noqa: E731
        return self._grown(call, room, cap, off), off

    def mismatches(self, bases, qual, info, offsets=None, patl: int = 0, n_reads: Optional[int] = None, max_patl: int = 0,
                   packed: bool = False, nflags=None, cap: int = 0):
        """real_hip_mismatches: the mismatch list of every placement among the records `info` (what match_unique returned for
        this batch) -> (lists, offsets): lists[offsets[i] : offsets[i + 1]] is read i's.  Host numpy arrays, device torch
        tensors (the outputs then are device tensors: int32 words of lib.MISMATCH_DTYPE, int64 offsets), or device reads with
        numpy records (on_device = 2)."""
        b, info = self._placed(bases, qual, info, offsets=offsets, patl=patl, n_reads=n_reads, max_patl=max_patl, packed=packed, nflags=nflags)
        n = int(b.n_reads)
        return self._mismatch_call(lambda o, c, no, po: self._L.real_hip_mismatches(self._h, C.byref(b), _ptr(info), o, c, no, po),
                                   n, not isinstance(info, np.ndarray), cap or max(1024, 4 * n))

    def mismatches_pairs(self, mate1, mate2, pairs, singles1=None, singles2=None, cap: int = 0):
        """real_hip_mismatches_pairs: the lists of both mates' final placements (mate 1 of fragment i is list 2i, mate 2 list
        2i + 1) from the pair records and, where given, the mates' single records; mates as (bases, qual, offsets) tuples or
        ReadBatch-like objects, all host arrays or all device tensors"""
        b1, b2, pairs, singles1, singles2 = self._placed_pairs(mate1, mate2, pairs, singles1, singles2)
        n = int(b1.n_reads)
        return self._mismatch_call(lambda o, c, no, po: self._L.real_hip_mismatches_pairs(
            self._h, C.byref(b1), C.byref(b2), _ptr(pairs), _ptr(singles1), _ptr(singles2), o, c, no, po),
            2 * n, not isinstance(pairs, np.ndarray), cap or max(1024, 8 * n))

    def mismatch_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipMismatchStats, self._L.real_hip_mismatch_stats_get, reset)

    # -- duplicate marking: read summaries, then the marks of the placed reads / fragments (include/real_hip.h, "duplicates") --
    def read_summary(self, bases, qual, offsets=None, patl: int = 0, n_reads: Optional[int] = None, max_patl: int = 0,
                     packed: bool = False, nflags=None, min_qual: int = 15, out=None):
        """real_hip_read_summary: {len, qsum} of every read as lib.READ_SUM_DTYPE.  Host numpy arrays give a numpy array;
        device torch tensors give a device tensor of n x 2 int32 words (len, qsum), or -- out: a numpy array -- host records
        from device reads (on_device = 2)."""
        on_device = bool(getattr(bases, "is_cuda", False))
        host_out = not on_device or isinstance(out, np.ndarray)
        b = self._read_batch(bases, qual, offsets, patl=patl, n_reads=n_reads, max_patl=max_patl, packed=packed, nflags=nflags,
                             host_records=host_out)
        n = int(b.n_reads)
        if out is None:
            if host_out:
                out = np.zeros(n, dtype=_lib.READ_SUM_DTYPE)
            else:
                import torch
                out = torch.zeros((n, 2), dtype=torch.int32, device=bases.device)
        self.sync_inputs(out)
        self._check(self._L.real_hip_read_summary(self._h, C.byref(b), int(min_qual), _ptr(out)))
        return out

    def _mark_call(self, entry, records, sums, dtype):
        """one marking call: numpy records and summaries give numpy marks (on_device 0), device tensors a device uint8 tensor"""
        host = isinstance(records, np.ndarray)
        if host:
            records = np.ascontiguousarray(records, dtype=dtype)
            sums = [np.ascontiguousarray(s, dtype=_lib.READ_SUM_DTYPE) for s in sums]
            n = int(records.shape[0])
            dup = np.zeros(n, dtype=np.uint8)
        else:
            import torch
            n = int(records.shape[0])
            dup = torch.zeros(n, dtype=torch.uint8, device=records.device)
        if any(int(s.shape[0]) != n for s in sums):
            raise ValueError("one summary per record")
        self.sync_inputs(records, *sums, dup)
        self._check(entry(self._h, _ptr(records), *[_ptr(s) for s in sums], n, int(not host), _ptr(dup)))
        return dup

    def mark_duplicates(self, info, sums):
        """real_hip_mark_duplicates: dup[i] = 1 iff read i is placed and not its group's representative.  info: the records
        of match_unique (numpy uint64, or a device tensor of n 64-bit words), sums: what read_summary returned for them"""
        return self._mark_call(self._L.real_hip_mark_duplicates, info, [sums], np.uint64)

    def mark_duplicates_gapped(self, info, gaps, sums):
        """real_hip_mark_duplicates_gapped: the joint marking of a single-end run -- read i is placed by its info word or, where
        that places nothing, by its Unique gap record (match_gapped's), and both kinds meet in one group per 5' end.  info and
        sums as for mark_duplicates, gaps as lib.GAP_PLACE_DTYPE (or a device tensor holding the 16-byte records, first
        dimension n): all numpy or all device tensors"""
        host = isinstance(info, np.ndarray)
        if host != isinstance(gaps, np.ndarray):
            raise ValueError("info words and gap records live on one side: all numpy or all device tensors")
        if host:
            gaps = np.ascontiguousarray(gaps, dtype=_lib.GAP_PLACE_DTYPE)
        if int(gaps.shape[0]) != int(info.shape[0]):
            raise ValueError("one gap record per info word")
        self.sync_inputs(gaps)
        return self._mark_call(lambda h, rec, *rest: self._L.real_hip_mark_duplicates_gapped(h, rec, _ptr(gaps), *rest), info, [sums], np.uint64)

    def mark_duplicates_pairs(self, pairs, sums1, sums2):
        """real_hip_mark_duplicates_pairs: one byte per fragment; pairs as lib.PAIR_DTYPE (or a device tensor holding the
        records, first dimension n), sums1 / sums2 the two mates' summaries"""
        return self._mark_call(self._L.real_hip_mark_duplicates_pairs, pairs, [sums1, sums2], _lib.PAIR_DTYPE)

    def dup_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipDupStats, self._L.real_hip_dup_stats_get, reset)

    # -- mapping quality (real_hip_mapq_acc accumulators; include/real_hip.h, "mapping quality") --
    new_mapq_acc = staticmethod(new_mapq_acc)

    def mapq_hits(self, hits, off, acc=None, fresh: Optional[bool] = None):
        """real_hip_mapq_hits: the fold alone, on one read's lists as the caller holds them (numpy arrays of lib.HIT_DTYPE /
        uint64, or device torch tensors of the same layout; device inputs need `acc` as a device tensor of 40-byte records)."""
        on_device, n, ((hits, off, _),) = _held_lists([(hits, off, None)], "the offsets describe another number of reads")
        acc, fresh = _start_or_fold(acc, fresh, on_device, lambda: new_mapq_acc(n), "accumulators")
        self.sync_inputs(hits, off, acc)
        self._check(self._L.real_hip_mapq_hits(self._h, _ptr(hits), _ptr(off), n, int(on_device), int(fresh), _ptr(acc)))
        return acc

    def match_mapq(self, bases, qual, offsets=None, patl: int = 0, acc=None, n_reads: Optional[int] = None, max_patl: int = 0,
                   fresh: Optional[bool] = None):
        """real_hip_match_mapq: matchAll of the batch with the hits kept on the device, folded into acc (None starts them)."""
        b = self._read_batch(bases, qual, offsets, patl=patl, n_reads=n_reads, max_patl=max_patl)
        acc, fresh = _start_or_fold(acc, fresh, bool(b.on_device), lambda: new_mapq_acc(int(b.n_reads)), "accumulators")
        b.fresh = int(fresh)
        self.sync_inputs(acc)
        self._check(self._L.real_hip_match_mapq(self._h, C.byref(b), _ptr(acc)))
        return acc

    def mapq(self, info, score, acc):
        """real_hip_mapq: one byte per read from the final records of match_unique and the accumulators (numpy arrays give a
        numpy uint8 array, device tensors a device uint8 tensor); score may be None with scores off"""
        host = isinstance(info, np.ndarray)
        n = int(info.shape[0])
        if host:
            info = np.ascontiguousarray(info, dtype=np.uint64)
            score = None if score is None else np.ascontiguousarray(score, dtype=np.float32)
            acc = np.ascontiguousarray(acc, dtype=_lib.MAPQ_ACC_DTYPE)
            out = np.zeros(n, dtype=np.uint8)
        else:
            import torch
            out = torch.zeros(n, dtype=torch.uint8, device=info.device)
        self.sync_inputs(info, score, acc, out)
        self._check(self._L.real_hip_mapq(self._h, _ptr(info), _ptr(score), _ptr(acc), n, int(not host), _ptr(out)))
        return out

    def mapq_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipMapqStats, self._L.real_hip_mapq_stats_get, reset)

    # -- instrumentation --
    def counters(self, reset: bool = False) -> dict:
        c = RealHipCounters()
        self._check(self._L.real_hip_counters_get(self._h, C.byref(c), int(reset)))
        return c.as_dict()

    def kernel_time(self, which: int, reset: bool = False) -> Tuple[float, int]:
        ms = C.c_double(0)
        n = C.c_uint64(0)
        self._check(self._L.real_hip_kernel_time(self._h, which, C.byref(ms), C.byref(n), int(reset)))
        return float(ms.value), int(n.value)

    def timing_enable(self, on: bool):
        self._check(self._L.real_hip_timing_enable(self._h, int(on)))


# The reference's names for the two per-read matchers; the policy (fold vs. collect) is the
# only difference, exactly as UpdateUniqueInfo / VectorUpdater are for ::match.
class UniqueMatcher(HipMatcher):
    def match(self, bases, qual, offsets=None, patl: int = 0, info=None, score=None, **kw):
        return self.match_unique(bases, qual, offsets, patl, info, score, **kw)


class AllMatcher(HipMatcher):
    def match(self, bases, qual, offsets=None, patl: int = 0, **kw):
        return self.match_all(bases, qual, offsets, patl, **kw)

    # -- anchored gap placement: a single read with one insertion or deletion, placed around the hits of its two ends --
    new_gap_place = staticmethod(new_gap_place)

    @staticmethod
    def _gap_params(max_gap: int = 8, min_flank: int = 8, cost_mismatch: int = 4, cost_open: int = 6, cost_extend: int = 1,
                    max_cost: Optional[int] = None, margin: int = 0, totalkmax: int = 0) -> "_lib.RealHipGapParams":
        """the command line's defaults: costs 4 / 6 / 1, max_cost = 4 * (-e) + 6 + max_gap"""
        if max_cost is None:
            max_cost = 4 * int(totalkmax) + 6 + int(max_gap)
        return _lib.sized(_lib.RealHipGapParams, max_gap=int(max_gap), min_flank=int(min_flank), cost_mismatch=int(cost_mismatch),
                          cost_open=int(cost_open), cost_extend=int(cost_extend), max_cost=int(max_cost), margin=int(margin))

    @staticmethod
    def _gap_anchor_params(anchor_len: int, max_anchors: int = 32) -> "_lib.RealHipGapAnchorParams":
        return _lib.sized(_lib.RealHipGapAnchorParams, anchor_len=int(anchor_len), max_anchors=int(max_anchors))

    def _gap_anchor_call(self, b: RealHipBatch, info, out, fresh: Optional[bool], anchor_len: int, max_anchors: int, gap: dict, call):
        """what gap_anchor_hits and match_gapped share: the records started or folded into, the two parameter structs, the call"""
        on_device = b.on_device == 1
        out, fresh = _start_or_fold(out, fresh, on_device, lambda: new_gap_place(int(b.n_reads)), "gap records")
        if not on_device:
            out = np.ascontiguousarray(out, dtype=_lib.GAP_PLACE_DTYPE)
            info = None if info is None else np.ascontiguousarray(info, dtype=np.uint64)
        gp = self._gap_params(**dict({"totalkmax": self.opts.totalkmax}, **gap))
        ap = self._gap_anchor_params(anchor_len, max_anchors)
        self.sync_inputs(info, out)
        self._check(call(C.byref(gp), C.byref(ap), C.byref(b), _ptr(info), int(fresh), _ptr(out)))
        return out

    def gap_anchor_hits(self, reads, hits, hit_offsets, anchor_len: int, info=None, out=None, fresh: Optional[bool] = None,
                        max_anchors: int = 32, **gap):
        """real_hip_gap_anchor_hits: reads (a batch-like object or a (bases, qual, offsets) tuple) whose FINAL info word is NoMatch
        (info None: all of them) placed with at most one insertion or deletion around the hits of their first and last
        anchor_len bases -> gap records (lib.GAP_PLACE_DTYPE).  hits / hit_offsets: the lists of the 2 n sub-reads as match_all
        returns them (numpy arrays with host reads or with numpy info / out, device tensors with device reads and records).
        out: records to fold into (another genome file's or index block's), None starts them.  Needs the text, not the index.
        gap: max_gap, min_flank, cost_mismatch, cost_open, cost_extend, max_cost, margin (_gap_params)."""
        host = isinstance(hits, np.ndarray)
        b = self._mate_batch(reads, host_records=host)
        if host:
            hits, hit_offsets = np.ascontiguousarray(hits, dtype=HIT_DTYPE), np.ascontiguousarray(hit_offsets, dtype=np.uint64)
        if int(hit_offsets.shape[0]) != 2 * int(b.n_reads) + 1:
            raise ValueError("the hit offsets describe another number of sub-reads than two per read")
        self.sync_inputs(hits, hit_offsets)
        return self._gap_anchor_call(b, info, out, fresh, anchor_len, max_anchors, gap, lambda gp, ap, bb, i, f, o: self._L.real_hip_gap_anchor_hits(
            self._h, gp, ap, bb, i, _ptr(hits), _ptr(hit_offsets), f, o))

    def match_gapped(self, reads, anchor_len: int, info=None, out=None, fresh: Optional[bool] = None, max_anchors: int = 32,
                     host_records: bool = False, **gap):
        """real_hip_match_gapped: gap_anchor_hits on the library's own matchAll of the eligible reads' sub-reads, everything in
        between left on the device.  Needs the text and a resident index block.  host_records: device reads with numpy info /
        out."""
        b = self._mate_batch(reads, host_records=host_records)
        return self._gap_anchor_call(b, info, out, fresh, anchor_len, max_anchors, gap, lambda gp, ap, bb, i, f, o: self._L.real_hip_match_gapped(
            self._h, gp, ap, bb, i, f, o))

    def gap_anchor_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipGapAnchorStats, self._L.real_hip_gap_anchor_stats_get, reset)


class PairMatcher(AllMatcher):
    """Paired-end reads: matchAll of both mates and the join of their hit lists on the device, one record per fragment
    (real_hip_pair; semantics in include/real_hip.h and DESIGN.md).  The reference has no paired-end mode."""

    @staticmethod
    def _pair_params(min_insert: int, max_insert: int, orientation: int = 0) -> "_lib.RealHipPairParams":
        return _lib.sized(_lib.RealHipPairParams, min_insert=int(min_insert), max_insert=int(max_insert), orientation=int(orientation))

    new_pair_info = staticmethod(new_pair_info)

    @staticmethod
    def _search_params(max_anchors: int = 0) -> "_lib.RealHipMateSearchParams":
        return _lib.sized(_lib.RealHipMateSearchParams, max_anchors=int(max_anchors))

    def match_pairs(self, mate1, mate2, min_insert: int, max_insert: int, pairs=None, orientation: int = 0,
                    mate_search: bool = False, max_anchors: int = 0, fresh: Optional[bool] = None):
        """real_hip_match_pairs: mate i of mate1 and of mate2 belong together.  pairs: records to fold into (another genome
        file's), None starts them.  Host batches give a numpy record array; device batches (torch tensors) need `pairs`
        as a device tensor of 40-byte records (fresh=True: output only).  mate_search: real_hip_match_pairs_search -- every
        hit's window is searched for a placement of the other mate the seeds missed (max_anchors: 0 = no limit)."""
        b1, b2 = self._mate_batch(mate1), self._mate_batch(mate2)
        pp = self._pair_params(min_insert, max_insert, orientation)
        pairs, fresh = _start_or_fold(pairs, fresh, bool(b1.on_device), lambda: new_pair_info(int(b1.n_reads)))
        b1.fresh = b2.fresh = int(fresh)
        self.sync_inputs(pairs)
        if mate_search:
            sp = self._search_params(max_anchors)
            self._check(self._L.real_hip_match_pairs_search(self._h, C.byref(b1), C.byref(b2), C.byref(pp), C.byref(sp), _ptr(pairs)))
        else:
            self._check(self._L.real_hip_match_pairs(self._h, C.byref(b1), C.byref(b2), C.byref(pp), _ptr(pairs)))
        return pairs

    def pair_search(self, mate1, mate2, hits1, off1, hits2, off2, min_insert: int, max_insert: int, fileid: int = 0, pairs=None,
                    max_anchors: int = 0, orientation: int = 0, fresh: Optional[bool] = None):
        """real_hip_pair_search: the mate search alone on anchors the caller holds (numpy arrays of lib.HIT_DTYPE / uint64
        with host batches, device torch tensors of the same layout with device batches); needs the text, not the index."""
        b1, b2 = self._mate_batch(mate1), self._mate_batch(mate2)
        on_device, n, ((hits1, off1, _), (hits2, off2, _)) = _held_lists(
            [(hits1, off1, None), (hits2, off2, None)], "the anchors' offsets and the batches describe different numbers of fragments", b1)
        pairs, fresh = _start_or_fold(pairs, fresh, on_device, lambda: new_pair_info(n))
        pp = self._pair_params(min_insert, max_insert, orientation)
        sp = self._search_params(max_anchors)
        self.sync_inputs(hits1, off1, hits2, off2, pairs)
        self._check(self._L.real_hip_pair_search(self._h, C.byref(pp), C.byref(sp), C.byref(b1), C.byref(b2), _ptr(hits1), _ptr(off1),
                                                 _ptr(hits2), _ptr(off2), int(fileid), int(fresh), _ptr(pairs)))
        return pairs

    def mate_search_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipMateSearchStats, self._L.real_hip_mate_search_stats_get, reset)

    def pair_hits(self, hits1, off1, len1, hits2, off2, len2, min_insert: int, max_insert: int, fileid: int = 0, pairs=None,
                  orientation: int = 0, fresh: Optional[bool] = None):
        """real_hip_pair_hits: the join alone, on hit lists the caller holds (numpy arrays of lib.HIT_DTYPE / uint64 /
        uint32, or device torch tensors of the same layout, all of one kind)."""
        on_device, n, (m1, m2) = _held_lists([(hits1, off1, len1), (hits2, off2, len2)], "the two mates' arrays describe different numbers of reads")
        pairs, fresh = _start_or_fold(pairs, fresh, on_device, lambda: new_pair_info(n))
        pp = self._pair_params(min_insert, max_insert, orientation)
        self.sync_inputs(*m1, *m2, pairs)
        self._check(self._L.real_hip_pair_hits(self._h, C.byref(pp), *map(_ptr, m1 + m2), n, int(fileid), int(on_device), int(fresh), _ptr(pairs)))
        return pairs

    # -- single placements of a mate (real_hip_single records) --
    new_single_info = staticmethod(new_single_info)

    def single_hits(self, hits, off, lens, fileid: int = 0, singles=None, fresh: Optional[bool] = None):
        """real_hip_single_hits: the fold alone, on one mate's lists as the caller holds them (numpy arrays of lib.HIT_DTYPE /
        uint64 / uint32, or device torch tensors of the same layout, all of one kind; device inputs need `singles` as a device
        tensor of 16-byte records)."""
        on_device, n, (m,) = _held_lists([(hits, off, lens)], "the offsets and the lengths describe different numbers of reads")
        singles, fresh = _start_or_fold(singles, fresh, on_device, lambda: new_single_info(n))
        self.sync_inputs(*m, singles)
        self._check(self._L.real_hip_single_hits(self._h, *map(_ptr, m), n, int(fileid), int(on_device), int(fresh), _ptr(singles)))
        return singles

    def match_pairs_singles(self, mate1, mate2, min_insert: int, max_insert: int, pairs=None, singles1=None, singles2=None,
                            orientation: int = 0, mate_search: bool = False, max_anchors: int = 0, fresh: Optional[bool] = None):
        """real_hip_match_pairs_singles: match_pairs (mate_search: with the search behind the join) and, in the same call,
        each mate's hit list folded into its own records -> (pairs, singles1, singles2).  The three arrays are started
        together (None) or folded into together; device batches need all three as device tensors (fresh=True: output only)."""
        b1, b2 = self._mate_batch(mate1), self._mate_batch(mate2)
        pp = self._pair_params(min_insert, max_insert, orientation)
        given = [x is not None for x in (pairs, singles1, singles2)]
        if any(given) and not all(given):
            raise ValueError("pairs, singles1 and singles2 are started together or folded into together")
        n, on_device = int(b1.n_reads), bool(b1.on_device)
        pairs, fresh = _start_or_fold(pairs, fresh, on_device, lambda: new_pair_info(n))
        (singles1, _), (singles2, _) = (_start_or_fold(s, fresh, on_device, lambda: new_single_info(n)) for s in (singles1, singles2))
        b1.fresh = b2.fresh = int(fresh)
        self.sync_inputs(pairs, singles1, singles2)
        sp = self._search_params(max_anchors) if mate_search else None
        self._check(self._L.real_hip_match_pairs_singles(self._h, C.byref(b1), C.byref(b2), C.byref(pp), C.byref(sp) if sp is not None else None,
                                                         _ptr(pairs), _ptr(singles1), _ptr(singles2)))
        return pairs, singles1, singles2

    # -- mapping quality of fragments --
    def mapq_pair_hits(self, hits1, off1, len1, hits2, off2, len2, min_insert: int, max_insert: int, acc=None, orientation: int = 0,
                       fresh: Optional[bool] = None):
        """real_hip_mapq_pair_hits: the fold of the concordant pairs alone, on hit lists the caller holds (as pair_hits)."""
        on_device, n, (m1, m2) = _held_lists([(hits1, off1, len1), (hits2, off2, len2)], "the two mates' arrays describe different numbers of reads")
        acc, fresh = _start_or_fold(acc, fresh, on_device, lambda: new_mapq_acc(n), "accumulators")
        pp = self._pair_params(min_insert, max_insert, orientation)
        self.sync_inputs(*m1, *m2, acc)
        self._check(self._L.real_hip_mapq_pair_hits(self._h, C.byref(pp), *map(_ptr, m1 + m2), n, int(on_device), int(fresh), _ptr(acc)))
        return acc

    def match_pairs_mapq(self, mate1, mate2, min_insert: int, max_insert: int, pairs=None, singles1=None, singles2=None, acc_pair=None,
                         acc1=None, acc2=None, orientation: int = 0, mate_search: bool = False, max_anchors: int = 0,
                         fresh: Optional[bool] = None):
        """real_hip_match_pairs_mapq: match_pairs_singles and, in the same call, the three folds of the mapping quality ->
        (pairs, singles1, singles2, acc_pair, acc1, acc2).  The six arrays are started together (None) or folded into together;
        device batches need all six as device tensors (fresh=True: output only)."""
        b1, b2 = self._mate_batch(mate1), self._mate_batch(mate2)
        pp = self._pair_params(min_insert, max_insert, orientation)
        given = [x is not None for x in (pairs, singles1, singles2, acc_pair, acc1, acc2)]
        if any(given) and not all(given):
            raise ValueError("pairs, singles and accumulators are started together or folded into together")
        n, on_device = int(b1.n_reads), bool(b1.on_device)
        pairs, fresh = _start_or_fold(pairs, fresh, on_device, lambda: new_pair_info(n))
        (singles1, _), (singles2, _) = (_start_or_fold(s, fresh, on_device, lambda: new_single_info(n)) for s in (singles1, singles2))
        accs = [_start_or_fold(a, fresh, on_device, lambda: new_mapq_acc(n), "accumulators")[0] for a in (acc_pair, acc1, acc2)]
        b1.fresh = b2.fresh = int(fresh)
        self.sync_inputs(pairs, singles1, singles2, *accs)
        sp = self._search_params(max_anchors) if mate_search else None
        self._check(self._L.real_hip_match_pairs_mapq(self._h, C.byref(b1), C.byref(b2), C.byref(pp), C.byref(sp) if sp is not None else None,
                                                      _ptr(pairs), _ptr(singles1), _ptr(singles2), *map(_ptr, accs)))
        return (pairs, singles1, singles2, *accs)

    def mapq_pairs(self, pairs, acc_pair, singles1=None, singles2=None, acc1=None, acc2=None):
        """real_hip_mapq_pairs: two bytes per fragment (mate 1, mate 2) from the final records and the accumulators; the
        singles and the mates' accumulators are given together or not at all"""
        host = isinstance(pairs, np.ndarray)
        if host:
            pairs = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
            acc_pair = np.ascontiguousarray(acc_pair, dtype=_lib.MAPQ_ACC_DTYPE)
            singles1, singles2 = (None if s is None else np.ascontiguousarray(s, dtype=SINGLE_DTYPE) for s in (singles1, singles2))
            acc1, acc2 = (None if a is None else np.ascontiguousarray(a, dtype=_lib.MAPQ_ACC_DTYPE) for a in (acc1, acc2))
            n = int(pairs.shape[0])
            out = np.zeros(2 * n, dtype=np.uint8)
        else:
            import torch
            n = int(pairs.numel() * pairs.element_size() // 40)
            out = torch.zeros(2 * n, dtype=torch.uint8, device=pairs.device)
        self.sync_inputs(pairs, singles1, singles2, acc_pair, acc1, acc2, out)
        self._check(self._L.real_hip_mapq_pairs(self._h, _ptr(pairs), _ptr(singles1), _ptr(singles2), _ptr(acc_pair), _ptr(acc1), _ptr(acc2),
                                                n, int(not host), _ptr(out)))
        return out

    # -- gap rescue: a mate with one insertion or deletion, placed beside its uniquely placed mate (_gap_params: AllMatcher's) --
    def gap_rescue(self, mate1, mate2, pairs, singles1, singles2, min_insert: int, max_insert: int, out=None, fresh: Optional[bool] = None,
                   orientation: int = 0, **gap):
        """real_hip_gap_rescue: per fragment whose pair record is NoMatch with one mate Unique on its own and the other nowhere,
        the other mate placed with at most one insertion or deletion inside the window the insert bounds allow -> gap records
        (lib.GAP_PLACE_DTYPE).  pairs / singles are the FINAL records (what match_pairs_singles left after all genome files);
        out: records to fold into (another genome file's), None starts them.  Needs the text of the genome file, not its index.
        gap: max_gap, min_flank, cost_mismatch, cost_open, cost_extend, max_cost, margin (_gap_params)."""
        b1, b2, pairs, singles1, singles2 = self._placed_pairs(mate1, mate2, pairs, singles1, singles2)
        host = isinstance(pairs, np.ndarray)
        out, fresh = _start_or_fold(out, fresh, not host, lambda: new_gap_place(int(b1.n_reads)), "gap records")
        if host:
            out = np.ascontiguousarray(out, dtype=_lib.GAP_PLACE_DTYPE)
        pp = self._pair_params(min_insert, max_insert, orientation)
        gp = self._gap_params(**dict({"totalkmax": self.opts.totalkmax}, **gap))
        self.sync_inputs(out)
        self._check(self._L.real_hip_gap_rescue(self._h, C.byref(pp), C.byref(gp), C.byref(b1), C.byref(b2), _ptr(pairs), _ptr(singles1),
                                                _ptr(singles2), int(fresh), _ptr(out)))
        return out

    def gap_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipGapStats, self._L.real_hip_gap_stats_get, reset)

    # -- gapped mismatch lists: where a rescued mate differs from the text, in the coordinates of its gapped placement --
    def mismatches_gapped(self, mate1, mate2, gaps, cap: int = 0):
        """real_hip_mismatches_gapped: list i is that of fragment i's gap record (what gap_rescue returned): the aligned bases
        of the record's target mate that differ from the text and the text bases its deletion skips (base =
        lib.MISMATCH_DELETED) -> (lists as lib.MISMATCH_DTYPE, offsets).  Mates and records as for mismatches_pairs: all host
        arrays, all device tensors, or device reads with numpy records"""
        b1, b2, gaps = self._gapped_records(mate1, mate2, gaps)
        n = int(b1.n_reads)
        return self._mismatch_call(lambda o, c, no, po: self._L.real_hip_mismatches_gapped(
            self._h, C.byref(b1), C.byref(b2), _ptr(gaps), o, c, no, po), n, not isinstance(gaps, np.ndarray), cap or max(1024, 4 * n))

    def gapped_list_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipGappedListStats, self._L.real_hip_gapped_list_stats_get, reset)

    # -- indel calls: the rescued mates' insertions and deletions over the finished pileup (include/real_hip.h, "indel calls") --
    def indel_begin(self):
        """real_hip_indel_begin: needs a finished pileup of the resident text; a second begin starts again"""
        self._check(self._L.real_hip_indel_begin(self._h))

    def indel_add(self, mate1, mate2, gaps):
        """real_hip_indel_add: the events of the Unique gapped records among `gaps` (what gap_rescue returned for these mates).
        Mates and records as for mismatches_gapped: all host arrays, all device tensors, or device reads with numpy records"""
        b1, b2, gaps = self._gapped_records(mate1, mate2, gaps)
        self._check(self._L.real_hip_indel_add(self._h, C.byref(b1), C.byref(b2), _ptr(gaps)))

    def indel_finish(self, min_call_qual: int = 20, min_alt: int = 2, min_depth: int = 4):
        """real_hip_indel_finish: the events grouped and genotyped -> (distinct events, calls).  May be called again with other
        thresholds"""
        p = _lib.sized(_lib.RealHipIndelParams, min_call_qual=int(min_call_qual), min_alt=int(min_alt), min_depth=int(min_depth))
        n_events, n_calls = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.real_hip_indel_finish(self._h, C.byref(p), C.byref(n_events), C.byref(n_calls)))
        return int(n_events.value), int(n_calls.value)

    def indel_events(self, cap: int = 1024) -> np.ndarray:
        """the distinct events as lib.INDEL_DTYPE, ascending (pos, gap, seq); the buffer grows once to the size the library reports"""
        return self._host_list(self._L.real_hip_indel_events, _lib.INDEL_DTYPE, cap)

    def indel_calls(self, cap: int = 1024) -> np.ndarray:
        """the calls among them as lib.INDEL_DTYPE, in the events' order; the buffer grows once"""
        return self._host_list(self._L.real_hip_indel_calls, _lib.INDEL_DTYPE, cap)

    def indel_end(self):
        self._check(self._L.real_hip_indel_end(self._h))

    def indel_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipIndelStats, self._L.real_hip_indel_stats_get, reset)

    # -- gapped placements in the pileup and the calls (include/real_hip.h, the block of that name) --
    def _gapped_records(self, mate1, mate2, gaps):
        """both mates' batches and the fragments' gap records for a stage -> (batch 1, batch 2, gaps): all host arrays, all device
        tensors, or device reads with numpy records, as for mismatches_gapped"""
        host = isinstance(gaps, np.ndarray)
        if host:
            gaps = np.ascontiguousarray(gaps, dtype=_lib.GAP_PLACE_DTYPE)
        b1, b2 = self._mate_batch(mate1, host_records=host), self._mate_batch(mate2, host_records=host)
        self.sync_inputs(gaps)
        return b1, b2, gaps

    def pileup_add_gapped(self, mate1, mate2, gaps):
        """real_hip_pileup_add_gapped: the Unique records among `gaps` (what gap_rescue returned for these mates, or match_gapped
        with the batch given as both mates) into the begun pileup: depth and alt on the aligned positions, not on the deleted ones"""
        b1, b2, gaps = self._gapped_records(mate1, mate2, gaps)
        self._check(self._L.real_hip_pileup_add_gapped(self._h, C.byref(b1), C.byref(b2), _ptr(gaps)))

    def call_add_gapped(self, mate1, mate2, gaps):
        """real_hip_call_add_gapped: the evidence of the same records over the sites of the finished pileup"""
        b1, b2, gaps = self._gapped_records(mate1, mate2, gaps)
        self._check(self._L.real_hip_call_add_gapped(self._h, C.byref(b1), C.byref(b2), _ptr(gaps)))

    def pileup_depth_gapped(self, first: int, count: int, out=None) -> np.ndarray:
        """gdepth[first .. first + count), the gapped placements' share of the depth, as numpy uint32 (out: a device torch tensor
        of count 32-bit words instead); zeros when no gapped add was made"""
        on_device = bool(getattr(out, "is_cuda", False))
        if out is None:
            out = np.zeros(int(count), dtype=np.uint32)
        self.sync_inputs(out)
        self._check(self._L.real_hip_pileup_depth_gapped(self._h, int(first), int(count), _ptr(out), int(on_device)))
        return out

    def pileup_gapped_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipPileupGappedStats, self._L.real_hip_pileup_gapped_stats_get, reset)

    def single_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipSingleStats, self._L.real_hip_single_stats_get, reset)

    # -- insert sizes: the histogram of the Unique fragments' outer distances, and the bounds it suggests --
    def insert_hist(self, pairs, len1, len2, n_bins: int, hist=None, fresh: Optional[bool] = None):
        """real_hip_pair_insert_hist: hist[d] = Unique records of `pairs` with outer distance d, the last bin what lies beyond
        (numpy arrays of lib.PAIR_DTYPE / uint32 give a numpy uint64 histogram; device torch tensors of the same layout, all
        of one kind, need `hist` as a device tensor of n_bins 64-bit counts).  hist given: the counts are added to it unless
        fresh=True."""
        on_device = bool(getattr(len1, "is_cuda", False))
        if not on_device:
            pairs = np.ascontiguousarray(pairs, dtype=_lib.PAIR_DTYPE)
            len1, len2 = np.ascontiguousarray(len1, dtype=np.uint32), np.ascontiguousarray(len2, dtype=np.uint32)
            n = int(pairs.shape[0])
        else:
            n = int(pairs.numel() * pairs.element_size() // 40)
        if int(len1.shape[0]) != n or int(len2.shape[0]) != n:
            raise ValueError("the records and the lengths describe different numbers of fragments")
        if hist is not None and not on_device and (not isinstance(hist, np.ndarray) or hist.dtype != np.uint64 or not hist.flags.c_contiguous):
            raise ValueError("hist must be a contiguous numpy uint64 array")
        hist, fresh = _start_or_fold(hist, fresh, on_device, lambda: np.zeros(int(n_bins), dtype=np.uint64), "histogram")
        if int(hist.shape[0]) != int(n_bins):
            raise ValueError("hist must hold n_bins counts")
        self.sync_inputs(pairs, len1, len2, hist)
        self._check(self._L.real_hip_pair_insert_hist(self._h, _ptr(pairs), _ptr(len1), _ptr(len2), n, int(on_device), int(fresh),
                                                      int(n_bins), _ptr(hist)))
        return hist

    @staticmethod
    def insert_bounds(hist, min_count: int = _lib.REAL_HIP_INSERT_MIN_COUNT, iqr_mult: int = 3) -> dict:
        """real_hip_insert_bounds: the quartiles of a histogram and the bounds q1 - iqr_mult * iqr .. q3 + iqr_mult * iqr.
        Raises RealHipError with status REAL_HIP_E_STATE (fewer than min_count records) or REAL_HIP_E_OVERFLOW (q3 in the
        overflow bin)."""
        if hasattr(hist, "cpu"):
            hist = hist.cpu().numpy().view(np.uint64)
        hist = np.ascontiguousarray(hist, dtype=np.uint64)
        est = _lib.sized(_lib.RealHipInsertEstimate)
        L = _lib.load()
        rc = L.real_hip_insert_bounds(hist.ctypes.data, int(hist.shape[0]), int(min_count), int(iqr_mult), C.byref(est))
        if rc != _lib.REAL_HIP_OK:
            raise RealHipError(rc, {_lib.REAL_HIP_E_STATE: "too few records for insert bounds (n = %d)" % est.n,
                                    _lib.REAL_HIP_E_OVERFLOW: "the third quartile lies in the overflow bin"}.get(rc, "invalid argument"))
        return {"n": int(est.n), "q1": int(est.q1), "median": int(est.median), "q3": int(est.q3), "low": int(est.low), "high": int(est.high)}

    def insert_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipInsertStats, self._L.real_hip_insert_stats_get, reset)

    def pair_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipPairStats, self._L.real_hip_pair_stats_get, reset)

    # -- every concordant pair of a fragment (real_hip_pair_hit records) --
    def _pair_all_call(self, call, n: int, on_device: bool, cap: int, out, pair_offsets):
        """one enumeration call: host outputs are allocated here and grow once to the size the library reports (_grown);
        device outputs are the caller's (a too small `out` raises, the error's .needed says how many records it takes)"""
        nout = C.c_uint64(0)
        if on_device:
            if out is None or pair_offsets is None:
                raise ValueError("device inputs need device tensors for the pair hits and the offsets")
            self.sync_inputs(out, pair_offsets)
            rc = call(_ptr(out), int(cap or out.numel() * out.element_size() // 32), C.byref(nout), _ptr(pair_offsets))
            if rc == _lib.REAL_HIP_E_OVERFLOW:      # the caller's tensor: he sizes it again (needed: records)
                err = RealHipError(rc, "pair hit buffer too small: %d records needed" % nout.value)
                err.needed = int(nout.value)
                raise err
            self._check(rc)
            return int(nout.value), pair_offsets
        poff = np.zeros(n + 1, dtype=np.uint64)
        return self._grown(call, lambda c: np.zeros(c, dtype=PAIR_HIT_DTYPE), cap or max(1024, 2 * n), poff), poff

    def pair_all_hits(self, hits1, off1, len1, hits2, off2, len2, min_insert: int, max_insert: int, fileid: int = 0,
                      orientation: int = 0, cap: int = 0, out=None, pair_offsets=None):
        """real_hip_pair_all_hits: every concordant pair of every fragment, row-major over the product of the two lists the
        caller holds.  Host arrays -> (pair hits as lib.PAIR_HIT_DTYPE, offsets); device tensors need `out` (32-byte
        records) and `pair_offsets` (n + 1 int64) as device tensors -> (number of pairs, pair_offsets)."""
        on_device, n, (m1, m2) = _held_lists([(hits1, off1, len1), (hits2, off2, len2)], "the two mates' arrays describe different numbers of reads")
        pp = self._pair_params(min_insert, max_insert, orientation)
        self.sync_inputs(*m1, *m2)

        def call(o, c, no, po):
            return self._L.real_hip_pair_all_hits(self._h, C.byref(pp), *map(_ptr, m1 + m2), n, int(fileid), int(on_device), o, c, no, po)
        return self._pair_all_call(call, n, on_device, cap, out, pair_offsets)

    def match_pairs_all(self, mate1, mate2, min_insert: int, max_insert: int, orientation: int = 0, cap: int = 0, out=None,
                        pair_offsets=None):
        """real_hip_match_pairs_all: matchAll of both mates with the hits kept on the device, then every concordant pair.
        Host batches -> (pair hits, offsets) as numpy arrays; device batches need `out` and `pair_offsets` as device
        tensors -> (number of pairs, pair_offsets)."""
        b1, b2 = self._mate_batch(mate1), self._mate_batch(mate2)
        pp = self._pair_params(min_insert, max_insert, orientation)

        def call(o, c, no, po):
            return self._L.real_hip_match_pairs_all(self._h, C.byref(b1), C.byref(b2), C.byref(pp), o, c, no, po)
        return self._pair_all_call(call, int(b1.n_reads), bool(b1.on_device), cap, out, pair_offsets)

    def pair_all_stats(self, reset: bool = False) -> dict:
        return self._stats(_lib.RealHipPairAllStats, self._L.real_hip_pair_all_stats_get, reset)
