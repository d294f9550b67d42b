"""The Python mirror of include/real_hip.h without a GPU: every struct of the header against its ctypes.Structure in
real_amd/lib.py (abi_header.header_structs() is the one parser, the per-feature abi tests share it), and the five helpers every wrapper of
real_amd/matcher.py goes through -- the batch builder, the growing list, start-or-fold, the caller-held lists, sized structs
and the statistics read -- on host arrays and fake calls."""
import ctypes as C

import numpy as np
import pytest

from abi_header import header_structs, mirror_of
from real_amd import lib as rlib
from real_amd.matcher import (HipMatcher, PairMatcher, _held_lists, _start_or_fold, new_pair_info)


# the records lib.py holds as numpy dtypes alone
DTYPES = {"real_hip_hit": rlib.HIT_DTYPE, "real_hip_pair": rlib.PAIR_DTYPE, "real_hip_single": rlib.SINGLE_DTYPE,
          "real_hip_call_evidence_rec": rlib.CALL_EVIDENCE_DTYPE, "real_hip_call": rlib.CALL_DTYPE}
# records with a ctypes.Structure and the dtype derived from it
TWINS = {"real_hip_pileup_site": rlib.PILEUP_SITE_DTYPE, "real_hip_mismatch": rlib.MISMATCH_DTYPE, "real_hip_read_sum": rlib.READ_SUM_DTYPE,
         "real_hip_pair_hit": rlib.PAIR_HIT_DTYPE}


def test_parser_copes_with_arrays_pointers_and_lists():
    hs = header_structs()
    assert hs["real_hip_params"][-2:] == ["filter_mult", "LL"] and hs["real_hip_pileup_site"] == ["pos", "depth", "alt", "ref", "reserved"]
    assert hs["real_hip_batch"] == ["struct_size", "on_device", "n_reads", "bases", "qual", "offsets", "patl", "max_patl", "packed", "fresh", "nflags"]
    assert hs["real_hip_call"] == ["pos", "depth", "cnt", "qual", "ref", "a1", "a2", "gq"]
    assert hs["real_hip_build_stats"][:3] == ["struct_size", "reserved", "wall_ms"] and "real_hip_ctx" not in hs
    assert len(hs) >= 28, sorted(hs)


def test_every_struct_of_the_header_against_its_mirror():
    hs = header_structs()
    mirrored = 0
    for name, names in hs.items():
        cls = mirror_of(name)
        if names[0] == "struct_size":
            assert cls is not None, "%s starts with struct_size and has no ctypes.Structure in lib.py" % name
        if cls is not None:
            assert [f for f, _ in cls._fields_] == names, name
            mirrored += 1
        if name in DTYPES or name in TWINS:
            assert list({**DTYPES, **TWINS}[name].names) == names, name
        assert cls is not None or name in DTYPES, "%s is mirrored neither as a Structure nor as a dtype" % name
    assert mirrored == len(hs) - len(DTYPES)
    for name, dtype in TWINS.items():       # written once: the dtype is the Structure's, offsets and size with it
        cls = mirror_of(name)
        assert dtype == np.dtype(cls) and dtype.itemsize == C.sizeof(cls)
        assert [dtype.fields[f][1] for f in dtype.names] == [getattr(cls, f).offset for f in dtype.names], name


# ---- the batch builder -----------------------------------------------------------------------------------------------
def _strided(a):
    """the values of `a` as every other element of an array twice as long: not contiguous"""
    wide = np.repeat(a, 2)
    wide[1::2] += 1
    v = wide[::2]
    assert not v.flags.c_contiguous and np.array_equal(v, a)
    return v


def test_read_batch_makes_host_arrays_contiguous_and_keeps_them():
    bases = np.arange(150, dtype=np.uint8) % 4
    qual = (np.arange(150, dtype=np.uint8) * 7) % 64
    offsets = np.array([0, 50, 100, 150], dtype=np.uint64)
    b = HipMatcher._read_batch(_strided(bases), _strided(qual), _strided(offsets))
    kb, kq, ko, kn = b._keep
    assert kn is None and (kb.dtype, kq.dtype, ko.dtype) == (np.uint8, np.uint8, np.uint64)
    assert all(k.flags.c_contiguous for k in (kb, kq, ko))
    assert np.array_equal(kb, bases) and np.array_equal(kq, qual) and np.array_equal(ko, offsets)
    assert (b.bases, b.qual, b.offsets) == (kb.ctypes.data, kq.ctypes.data, ko.ctypes.data)
    assert b.struct_size == C.sizeof(rlib.RealHipBatch) and b.on_device == 0 and b.n_reads == 3
    assert (b.patl, b.max_patl, b.packed, b.fresh, b.nflags) == (0, 0, 0, 0, None)
    # other integer types are converted, a contiguous array of the right type is used where it lies
    b = HipMatcher._read_batch(bases.astype(np.int64), None, offsets.astype(np.int32))
    assert b._keep[0].dtype == np.uint8 and b._keep[2].dtype == np.uint64 and b.qual is None and b.n_reads == 3
    b = HipMatcher._read_batch(bases, qual, offsets)
    assert (b.bases, b.qual, b.offsets) == (bases.ctypes.data, qual.ctypes.data, offsets.ctypes.data)


def test_read_batch_counts_reads_and_fills_the_flags():
    bases = np.zeros(150, dtype=np.uint8)
    assert HipMatcher._read_batch(bases, None, patl=50).n_reads == 3                   # from patl
    assert HipMatcher._read_batch(bases, None, patl=50, n_reads=2).n_reads == 2        # as said
    assert HipMatcher._read_batch(bases, None, np.array([0, 150], dtype=np.uint64), n_reads=7).n_reads == 1    # the offsets decide
    with pytest.raises(ValueError, match="a packed batch of uniform length needs n_reads"):
        HipMatcher._read_batch(bases, None, patl=50, packed=True)
    nflags = np.zeros(75, dtype=np.uint8)
    b = HipMatcher._read_batch(bases, None, patl=8, n_reads=75, packed=True, nflags=nflags, fresh=True, max_patl=9)
    assert (b.n_reads, b.patl, b.max_patl, b.packed, b.fresh, b.nflags, b.on_device) == (75, 8, 9, 1, 1, nflags.ctypes.data, 0)
    assert b._keep[3] is nflags
    assert HipMatcher._read_batch(bases, None, patl=50, host_records=True).on_device == 0      # host reads are host reads
    # raw addresses (what parse_reads returns): the caller says where they lie and how many reads they are
    b = HipMatcher._read_batch(4096, None, 8192, n_reads=5, max_patl=100, on_device=2)
    assert (b.bases, b.qual, b.offsets, b.n_reads, b.max_patl, b.on_device) == (4096, None, 8192, 5, 100, 2)
    # the same through the innermost step, as bench.py calls it
    b = HipMatcher._batch(bases, None, None, 50, 3)
    assert (b.struct_size, b.n_reads, b.patl, b.bases, b.on_device) == (C.sizeof(rlib.RealHipBatch), 3, 50, bases.ctypes.data, 0)


def test_read_batch_never_copies_a_submitted_array():
    bases, qual = np.zeros(100, dtype=np.uint8), np.zeros(100, dtype=np.uint8)
    b = HipMatcher._read_batch(bases, qual, patl=50, on_device=0, copy=False)
    assert b._keep[0] is bases and b._keep[1] is qual and (b.bases, b.qual) == (bases.ctypes.data, qual.ctypes.data)
    with pytest.raises(ValueError, match="contiguous"):
        HipMatcher._read_batch(_strided(bases), qual, patl=50, on_device=0, copy=False)
    with pytest.raises(ValueError, match="contiguous"):
        HipMatcher._read_batch(bases, _strided(qual), patl=50, on_device=0, copy=False)


def test_mate_batch_takes_tuples_and_batch_objects():
    import types
    bases, offsets = np.zeros(100, dtype=np.uint8), np.array([0, 40, 100], dtype=np.uint64)
    m = _bare_matcher()
    for mate in ((bases, None, offsets), types.SimpleNamespace(bases=bases, qual=None, offsets=offsets)):
        b = m._mate_batch(mate, fresh=True)
        assert (b.n_reads, b.bases, b.offsets, b.fresh) == (2, bases.ctypes.data, offsets.ctypes.data, 1)


# ---- the growing list ------------------------------------------------------------------------------------------------
class _FakeLibrary:
    @staticmethod
    def real_hip_last_error(h):
        return b""

    @staticmethod
    def real_hip_strerror(rc):
        return b"status %d" % rc


def _bare_matcher(cls=HipMatcher):
    """a matcher without a context: what the helpers need of one is _check"""
    m = cls.__new__(cls)
    m._L, m._h = _FakeLibrary(), None
    return m


def _list_call(total, statuses, calls):
    """a list entry point of the library: reports `total` records, writes them when they fit, returns the next of `statuses`"""
    def call(out, cap, n_out, offsets):
        calls.append((out, cap, offsets))
        n_out._obj.value = total
        if cap >= total:
            C.memmove(out, np.arange(total, dtype=np.uint32).ctypes.data, 4 * total)
        return statuses[len(calls) - 1]
    return call


def _room(made):
    def room(cap):
        made.append(np.full(cap, 99, dtype=np.uint32))
        return made[-1]
    return room


def test_grown_fits_the_first_time():
    calls, made, off = [], [], np.zeros(3, dtype=np.uint64)
    out = _bare_matcher()._grown(_list_call(5, [0], calls), _room(made), 8, off)
    assert len(calls) == 1 and calls[0] == (made[0].ctypes.data, 8, off.ctypes.data)
    assert out.tolist() == [0, 1, 2, 3, 4] and out.base is made[0]


def test_grown_overflows_once_and_is_cut_to_the_count():
    calls, made = [], []
    out = _bare_matcher()._grown(_list_call(5, [rlib.REAL_HIP_E_OVERFLOW, 0], calls), _room(made), 2)
    assert [(c[1], c[2]) for c in calls] == [(2, None), (5, None)] and [len(a) for a in made] == [2, 5]
    assert calls[1][0] == made[1].ctypes.data and out.tolist() == [0, 1, 2, 3, 4]
    calls, made = [], []                    # a count below the second capacity cuts the result
    out = _bare_matcher()._grown(_list_call(3, [0], calls), _room(made), 1024)
    assert len(out) == 3 and len(made[0]) == 1024


def test_grown_raises_a_second_overflow():
    calls, made = [], []
    with pytest.raises(rlib.RealHipError) as e:
        _bare_matcher()._grown(_list_call(5, [rlib.REAL_HIP_E_OVERFLOW] * 4, calls), _room(made), 2)
    assert e.value.status == rlib.REAL_HIP_E_OVERFLOW and len(calls) == 2 and calls[1][1] == 5


def test_grown_raises_another_status_at_once():
    calls, made = [], []
    with pytest.raises(rlib.RealHipError) as e:
        _bare_matcher()._grown(_list_call(5, [rlib.REAL_HIP_E_INVALID, 0], calls), _room(made), 8)
    assert e.value.status == rlib.REAL_HIP_E_INVALID and len(calls) == 1


# ---- start or fold, caller-held lists ------------------------------------------------------------------------------------
def test_start_or_fold():
    made = []

    def new():
        made.append(new_pair_info(3))
        return made[-1]
    rec, fresh = _start_or_fold(None, None, False, new)
    assert rec is made[0] and fresh is True
    rec, fresh = _start_or_fold(None, False, False, new)            # started, and the caller says the start is to be folded into
    assert rec is made[1] and fresh is False
    given = new_pair_info(3)
    rec, fresh = _start_or_fold(given, None, False, new)
    assert rec is given and fresh is False
    rec, fresh = _start_or_fold(given, True, True, new)             # output only
    assert rec is given and fresh is True and len(made) == 2
    with pytest.raises(ValueError, match="device inputs need a device tensor for the records"):
        _start_or_fold(None, None, True, new)
    with pytest.raises(ValueError, match="device inputs need a device tensor for the histogram"):
        _start_or_fold(None, True, True, new, "histogram")
    assert len(made) == 2


def test_held_lists():
    hits = np.zeros(8, dtype=rlib.HIT_DTYPE)
    hits["pos"] = np.arange(8)
    off, lens = np.array([0, 3, 8], dtype=np.int64), np.array([50, 60], dtype=np.int64)
    on_device, n, ((h, o, ln), (h2, o2, l2)) = _held_lists([(hits[::2], _strided(off), lens), (hits, off, lens)], "differ")
    assert (on_device, n) == (False, 2) and (h.dtype, o.dtype, ln.dtype) == (rlib.HIT_DTYPE, np.uint64, np.uint32)
    assert h.flags.c_contiguous and h["pos"].tolist() == [0, 2, 4, 6] and o.tolist() == [0, 3, 8] and ln.tolist() == [50, 60]
    assert h2 is hits and o2.dtype == np.uint64
    with pytest.raises(ValueError, match="differ"):
        _held_lists([(hits, off, lens), (hits, off[:2], lens)], "differ")
    with pytest.raises(ValueError, match="differ"):
        _held_lists([(hits, off, lens[:1])], "differ")
    # lists that come with a batch: the batch's count, no lengths
    batch = HipMatcher._read_batch(np.zeros(100, dtype=np.uint8), None, patl=50)
    assert _held_lists([(hits, off, None)], "differ", batch)[:2] == (False, 2)
    with pytest.raises(ValueError, match="differ"):
        _held_lists([(hits, off[:2], None)], "differ", batch)


# ---- sized structs, statistics -----------------------------------------------------------------------------------------
def test_sized_sets_struct_size_and_the_fields():
    for cls in (rlib.RealHipParams, rlib.RealHipBatch, rlib.RealHipPairParams, rlib.RealHipMateSearchParams, rlib.RealHipPileupParams,
                rlib.RealHipCallParams, rlib.RealHipInsertEstimate, rlib.RealHipDupStats):
        assert rlib.sized(cls).struct_size == C.sizeof(cls) > 0
    p = rlib.sized(rlib.RealHipCallParams, min_call_qual=20, min_depth=4)
    assert (p.struct_size, p.min_call_qual, p.min_depth) == (12, 20, 4)
    pp = PairMatcher._pair_params(150, 420, 1)
    assert (pp.struct_size, pp.min_insert, pp.max_insert, pp.orientation) == (16, 150, 420, 1)
    sp = PairMatcher._search_params(7)
    assert (sp.struct_size, sp.max_anchors, list(sp.reserved)) == (16, 7, [0, 0])


# what every *_stats() reported before its field names were taken from the struct: written out, that is the point
STATS_KEYS = {
    "index_build_stats": (rlib.RealHipBuildStats, ("wall_ms", "kernel_ms", "alloc_ms", "free_ms", "alloc_bytes", "alloc_calls", "free_calls")),
    "pileup_stats": (rlib.RealHipPileupStats, ("reads", "placed", "other_file", "invalid", "bases", "mismatches", "low_qual", "n_dropped",
                                                "covered", "sites", "max_depth", "launches", "kernel_ms")),
    "call_stats": (rlib.RealHipCallStats, ("reads", "placed", "other_file", "invalid", "site_bases", "low_qual", "calls", "het", "hom",
                                            "launches", "kernel_ms")),
    "mismatch_stats": (rlib.RealHipMismatchStats, ("reads", "placed", "other_file", "invalid", "bases", "mismatches", "on_n", "disagree",
                                                    "launches", "kernel_ms")),
    "dup_stats": (rlib.RealHipDupStats, ("reads", "placed", "groups", "duplicates", "launches", "kernel_ms")),
    "mate_search_stats": (rlib.RealHipMateSearchStats, ("fragments", "anchors", "anchors_skipped", "positions", "placements", "launches",
                                                         "kernel_ms")),
    "single_stats": (rlib.RealHipSingleStats, ("reads", "hits", "handed_over", "launches", "kernel_ms")),
    "insert_stats": (rlib.RealHipInsertStats, ("records", "counted", "overflow", "invalid", "launches", "kernel_ms")),
    "pair_stats": (rlib.RealHipPairStats, ("pairs", "products", "handed_over")),
    "pair_all_stats": (rlib.RealHipPairAllStats, ("fragments", "products", "pairs_out", "handed_over", "launches", "kernel_ms")),
}


@pytest.mark.parametrize("method", sorted(STATS_KEYS))
def test_stats_keys(method):
    struct, keys = STATS_KEYS[method]
    seen = []

    def entry(h, st, reset):
        """fills field i with i + 1 (i + 1.5 for a time) and checks the struct announces its size"""
        st = st._obj
        assert st.struct_size == C.sizeof(struct) and st.reserved == 0
        for i, (k, t) in enumerate(struct._fields_[2:]):
            setattr(st, k, i + (1.5 if t is C.c_double else 1))
        seen.append(reset)
        return 0
    m = _bare_matcher(PairMatcher)
    m._L = type("L", (_FakeLibrary,), {"real_hip_%s" % f: staticmethod(entry) for f in (
        "index_build_stats", "pileup_stats_get", "call_stats_get", "mismatch_stats_get", "dup_stats_get", "mate_search_stats_get",
        "single_stats_get", "insert_stats_get", "pair_stats_get", "pair_all_stats_get")})()
    got = getattr(m, method)(reset=True)
    assert tuple(got) == keys and seen == [1]
    for i, k in enumerate(keys):
        assert got[k] == i + (1.5 if k.endswith("_ms") else 1) and type(got[k]) is (float if k.endswith("_ms") else int), k
    assert rlib.stats_fields(struct) == keys and C.sizeof(struct) == 8 + 8 * len(keys)
