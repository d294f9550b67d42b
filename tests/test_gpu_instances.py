"""The instance matrix: every compiled instance of the lane matcher, match_kernel<W, SCORES, ALL, TK, PASS2>
(match_kernel.hip; one translation unit per read width W = 1..10 words of 32 bases), and the wave matcher's LONG form in
every index layout, against the oracle on one shared genome.

One cell is one (width, geometry, scores on / off, matchUnique / matchAll).  The five index geometries give the four
table kinds of the lane matcher (TK_STARTS, TK_DIRECTORY twice -- digest and fingerprint --, TK_ROWS, TK_ROWS_WIDE); the
second-pass instances (bucket rows with scores on or matchAll) run wherever the six-copy family overflows the first
pass' parked locations.  Every call is compared bit for bit: records and score bits, matchAll hit lists with every
field, and the five work counters; every call also hands reads over to the wave matcher (the 60-copy family: equal
ranges longer than BIG_T).  A cell that differs from the oracle is a bug in the kernel, not in the matrix.

Left out: cells whose read cannot hold a seed (64-base seeds at W = 1), and bucket rows of 32-base seeds, which need
prefix_bits >= 28 (128 B x 2^28 rows x 6 lists, about 192 GB); the bench's GPU == CPU check over its whole read set is
their pin.  tests/test_instance_matrix.py checks on the CPU that the cells cover every compiled width and table kind.
"""
from dataclasses import dataclass

import numpy as np
import pytest

from real_amd import synth
from real_amd.lib import LAYOUT_DIGEST, LAYOUT_FINGERPRINT, LAYOUT_ROWS, LAYOUT_STARTS
from real_amd.matcher import NoMatch, NonUnique, RealOptions, Reverse, Straight, UniqueMatcher, unpack_info

pytestmark = pytest.mark.gpu

MAX_W = 10                      # REAL_HIP_MAX_PATL / 32 (tests/test_instance_matrix.py holds this to the header)
WORK = ("reads", "lookups", "candidates", "seedpass", "hits")
SEG = 760                       # repeat family segments: longer than any read that is drawn from them
FAMILIES = (3, 6, 30, 60)       # exact copies per family


@dataclass(frozen=True)
class Geometry:
    seedl: int
    table_kind: int             # the request (real_hip_params.table_kind)
    prefix_bits: int
    layout: int                 # what has to be built (an unmet request falls back silently)
    tk: str                     # the lane matcher's table kind for that layout


GEOMETRIES = {
    "starts": Geometry(32, 0, 0, LAYOUT_STARTS, "TK_STARTS"),
    "digest": Geometry(16, 0, 13, LAYOUT_DIGEST, "TK_DIRECTORY"),
    "fingerprint": Geometry(64, 2, 15, LAYOUT_FINGERPRINT, "TK_DIRECTORY"),
    "rows": Geometry(16, 3, 13, LAYOUT_ROWS, "TK_ROWS"),             # 32-bit signatures: pbits != 0
    "rows_wide": Geometry(64, 3, 15, LAYOUT_ROWS, "TK_ROWS_WIDE"),   # 64-bit signatures: pbits == 0
}
# (width, geometry) pairs that are not cells, and why
EXCLUDED = {(1, "fingerprint"): "a read of 32 bases cannot hold a 64-base seed",
            (1, "rows_wide"): "a read of 32 bases cannot hold a 64-base seed"}


@dataclass(frozen=True)
class Cell:
    w: int
    geom: str
    scores: int
    mode: str                   # "unique" | "all"

    @property
    def id(self):
        return "w%d-%s-%s-%s" % (self.w, self.geom, "scores" if self.scores else "noscores", self.mode)


CELLS = [Cell(w, geom, s, mode) for geom in GEOMETRIES for w in range(1, MAX_W + 1) if (w, geom) not in EXCLUDED
         for s in (1, 0) for mode in ("unique", "all")]

# ---------------------------------------------------------------------------------------------------------------------
# shared inputs (built once, on first use: collecting this module costs nothing)
# ---------------------------------------------------------------------------------------------------------------------
_cache = {}


def _genome():
    if "genome" not in _cache:
        _cache["genome"] = synth.repeat_family_genome(400_000, seed=2027, families=FAMILIES, seg_len=SEG, n_frag=4, n_runs=6)
    return _cache["genome"]


def _reads(seed, lengths, errs, rep_frac=1 / 3, rand_frac=0.05, n_every=40):
    """One read per entry of ``lengths``: a third from the repeat families (every 16th from the 60-copy one, every 16th
    from the 6-copy one), a few random (NoMatch), the rest from anywhere (N runs and fragment ends included); either
    strand; substitutions at ``errs(L)`` expected per read, plus a forced one at the first base of every 7th read and at
    the last base of the next; an N in every ``n_every``-th read; qualities 0..63, independent per base."""
    g, fam = _genome()
    rng = np.random.default_rng(seed)
    bases, quals = [], []
    for i, L in enumerate(int(x) for x in lengths):
        u = rng.random()
        f = 3 if i % 16 == 0 else 1 if i % 16 == 8 else int(rng.integers(len(FAMILIES))) if u < rep_frac else -1
        if f >= 0 and L <= SEG:
            c = fam[f][int(rng.integers(len(fam[f])))]
            r = g.sym[c + int(rng.integers(0, SEG - L + 1)):][:L].copy()
        elif u > 1 - rand_frac:
            r = rng.integers(0, 4, size=L, dtype=np.uint8)
        else:
            p = int(rng.integers(0, g.n - L + 1))
            r = g.sym[p:p + L].copy()
        if rng.random() < 0.5:
            r = synth.revcomp(r)
        mut = rng.random(L) < errs(L) / L
        if i % 7 == 1:
            mut[0] = True
        elif i % 7 == 2:
            mut[L - 1] = True
        r = np.where(mut & (r < 4), (r + rng.integers(1, 4, size=L)) & 3, r).astype(np.uint8)
        if i % n_every == n_every - 1:
            r[int(rng.integers(L))] = 4
        bases.append(r)
        quals.append(rng.integers(0, 64, size=L).astype(np.uint8))
    offsets = np.concatenate([[0], np.cumsum([b.shape[0] for b in bases])]).astype(np.uint64)
    return np.concatenate(bases), np.concatenate(quals), offsets


def _k(w):
    return min(15, 2 + w)


def _span(w, seedl):
    return max(seedl, 32 * w - 31), 32 * w


def _uniform(w, seedl):
    """650 reads (a partial last tile of 64) of 32W bases: every word full, the last-word mask all ones"""
    key = ("uniform", w, seedl)
    if key not in _cache:
        _cache[key] = _reads(10_000 + 100 * w + seedl, [32 * w] * 650, lambda L: _k(w) / 2)
    return _cache[key]


def _ragged(w, seedl):
    """every length of the width's span (so every residue mod 16 it holds), the longest first, and a few reads shorter
    than the seed (skipped)"""
    key = ("ragged", w, seedl)
    if key not in _cache:
        lo, hi = _span(w, seedl)
        rng = np.random.default_rng(20_000 + 100 * w + seedl)
        lens = [hi] + [lo + i % (hi - lo + 1) for i in range(300)] + list(rng.integers(max(4, seedl - 12), seedl, size=12))
        lens = [lens[0]] + list(rng.permutation(lens[1:]))
        _cache[key] = _reads(30_000 + 100 * w + seedl, lens, lambda L: _k(w) / 2)
    return _cache[key]


def _ora_index(ora, seedl):
    key = ("ora", seedl)
    if key not in _cache:
        g, _ = _genome()
        og = ora.Genome(g.sym, g.frag_start)
        _cache[key] = (og, ora.Index(og, seedl))
    return _cache[key]


def _oracle(ora, key, seedl, k, scores, mode, bases, qual, offsets, filter_level=2):
    """the oracle's answer, cached: it depends on the seed length, not on the table layout that serves it"""
    key = ("answer", seedl, k, scores, mode, filter_level) + key
    if key not in _cache:
        og, ix = _ora_index(ora, seedl)
        p = ora.make_params(seedl=seedl, seedkmax=2, totalkmax=k, scores=scores, filter_level=filter_level)
        f = ora.match_unique if mode == "unique" else ora.match_all
        _cache[key] = f(og, ix, p, bases, qual, offsets)
    return _cache[key]


@pytest.fixture(scope="module")
def matchers():
    """one context per geometry, its index built once; the cells switch -s / -e / -q with set_match_params"""
    made = {}

    def get(geom):
        if geom not in made:
            gm = GEOMETRIES[geom]
            g, _ = _genome()
            m = UniqueMatcher(RealOptions(seedl=gm.seedl, seedkmax=2, totalkmax=3).normalise(),
                              prefix_bits=gm.prefix_bits, table_kind=gm.table_kind)
            m.set_text_symbols(0, g.sym, g.frag_start)
            m.build_index_block()
            assert m.table_kind == gm.layout, (geom, m.table_kind)
            made[geom] = m
        return made[geom]

    yield get
    for m in made.values():
        m.close()


# ---------------------------------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------------------------------
def _first_diff(a, b):
    d = np.nonzero(a != b)[0]
    return "%d reads differ, first %d" % (d.shape[0], int(d[0])) if d.shape[0] else "equal"


def _check_counters(m, octr, what):
    c = m.counters()
    for kk in WORK:
        assert c[kk] == octr[kk], "%s: work counter %s %d != oracle %d" % (what, kk, c[kk], octr[kk])
    assert c["handed_over"] > 0, "%s: no read was handed over (the 60-copy family must be)" % what


def _unique(m, ora, okey, seedl, k, scores, bases, qual, offsets, what, patl=0, packed=False, filter_level=2):
    oinfo, oscore, octr = _oracle(ora, okey, seedl, k, scores, "unique", bases, qual, offsets, filter_level)
    m.counters(reset=True)
    if packed:
        info, score = m.match_unique(synth.pack_bases(bases), qual, offsets, packed=True,
                                     nflags=synth.read_nflags(bases, offsets))
    elif patl:
        info, score = m.match_unique(bases, qual, patl=patl)
    else:
        info, score = m.match_unique(bases, qual, offsets)
    assert np.array_equal(info, oinfo), "%s: records: %s" % (what, _first_diff(info, oinfo))
    if scores:
        sb, ob = score.view(np.uint32), oscore.view(np.uint32)
        assert np.array_equal(sb, ob), "%s: score bits: %s" % (what, _first_diff(sb, ob))
    _check_counters(m, octr, what)
    return info


def _all(m, ora, okey, seedl, k, scores, bases, qual, offsets, what, patl=0):
    ohits, ooff, octr = _oracle(ora, okey, seedl, k, scores, "all", bases, qual, offsets)
    m.counters(reset=True)
    cap = int(ohits.shape[0]) + 16                  # (no overflow retry: the work is counted once)
    if patl:
        hits, hoff = m.match_all(bases, qual, patl=patl, cap=cap)
    else:
        hits, hoff = m.match_all(bases, qual, offsets, cap=cap)
    assert np.array_equal(hoff, ooff), "%s: hits per read: %s" % (what, _first_diff(np.diff(hoff.astype(np.int64)), np.diff(ooff.astype(np.int64))))
    for f in ("read", "pos", "frag", "k", "inverted"):
        a, b = hits[f].astype(np.int64), ohits[f].astype(np.int64)
        assert np.array_equal(a, b), "%s: hit field %s: %d of %d differ" % (what, f, int((a != b).sum()), a.shape[0])
    sa, sb = hits["score"].view(np.uint32), ohits["score"].view(np.uint32)
    assert np.array_equal(sa, sb), "%s: hit score bits: %d of %d differ" % (what, int((sa != sb).sum()), sa.shape[0])
    _check_counters(m, octr, what)
    return hits


# ---------------------------------------------------------------------------------------------------------------------
# 1. the instance matrix
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", CELLS, ids=[c.id for c in CELLS])
def test_instance_matches_oracle(ora, matchers, cell):
    gm = GEOMETRIES[cell.geom]
    w, seedl, scores, k = cell.w, gm.seedl, cell.scores, _k(cell.w)
    m = matchers(cell.geom)
    m.set_match_params(seedkmax=2, totalkmax=k, scores=scores, filter_level=2)
    run = _unique if cell.mode == "unique" else _all
    ub, uq, uo = _uniform(w, seedl)
    n = uo.shape[0] - 1
    out = run(m, ora, ("uniform", w), seedl, k, scores, ub, uq, uo, cell.id + " uniform", patl=32 * w)
    if cell.mode == "unique":
        st = unpack_info(out)[0]
        assert ((st == Straight) | (st == Reverse)).sum() > 0 and (st == NonUnique).sum() > 0 and (st == NoMatch).sum() > 0, \
            "%s: the batch must hold unique, NonUnique and unmatched reads" % cell.id
    else:
        assert out.shape[0] > n // 2, "%s: %d matchAll hits for %d reads" % (cell.id, out.shape[0], n)
    rb, rq, ro = _ragged(w, seedl)
    run(m, ora, ("ragged", w), seedl, k, scores, rb, rq, ro, cell.id + " ragged")
    if cell.mode == "unique":           # reads that start inside a byte
        run(m, ora, ("ragged", w), seedl, k, scores, rb, rq, ro, cell.id + " ragged packed", packed=True)
    if scores:                          # reads without qualities: 30 each
        run(m, ora, ("uniform-noqual", w), seedl, k, scores, ub, None, uo, cell.id + " no qualities", patl=32 * w)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the wave matcher's LONG form in every layout
# ---------------------------------------------------------------------------------------------------------------------
LONG_CASES = [(geom, s, mode) for geom in GEOMETRIES for s in (1, 0) for mode in ("unique", "all")]


def _long_batch():
    if "long" not in _cache:
        rng = np.random.default_rng(40_000)
        lens = [100] * 150 + list(rng.integers(321, 701, size=40)) + list(rng.integers(1000, 1601, size=4))
        lens = list(rng.permutation(lens))
        _cache["long"] = _reads(40_001, lens, lambda L: 0.01 * L)
    return _cache["long"]


@pytest.mark.parametrize("geom,scores,mode", LONG_CASES,
                         ids=["long-%s-%s-%s" % (g, "scores" if s else "noscores", md) for g, s, md in LONG_CASES])
def test_long_reads_in_every_layout(ora, matchers, geom, scores, mode):
    """100 bp reads mixed with reads of 321..700 and 1000+ bases: the latter longer than any lane holds (a wave each,
    LONG form)"""
    gm = GEOMETRIES[geom]
    m = matchers(geom)
    m.set_match_params(seedkmax=2, totalkmax=15, scores=scores, filter_level=2)
    b, q, o = _long_batch()
    run = _unique if mode == "unique" else _all
    run(m, ora, ("long",), gm.seedl, 15, scores, b, q, o, "long-%s-%d-%s" % (geom, scores, mode))


@pytest.mark.parametrize("geom,scores", [(g, s) for g in GEOMETRIES for s in (1, 0)],
                         ids=["declared-%s-%s" % (g, "scores" if s else "noscores") for g in GEOMETRIES for s in (1, 0)])
def test_declared_max_patl_selects_the_long_form(ora, matchers, geom, scores):
    """Device-resident reads of 40..100 bases with max_patl = 32W declared, W = 4..10: instance W runs on reads far
    shorter than its registers, the wave matcher in its LONG form (real_hip_api.hip: a declared max_patl)"""
    import torch
    gm = GEOMETRIES[geom]
    m = matchers(geom)
    k = 6
    m.set_match_params(seedkmax=2, totalkmax=k, scores=scores, filter_level=2)
    if "short" not in _cache:
        _cache["short"] = _reads(50_000, np.random.default_rng(50_001).integers(40, 101, size=400), lambda L: 0.02 * L)
    b, q, o = _cache["short"]
    oinfo, oscore, octr = _oracle(ora, ("short",), gm.seedl, k, scores, "unique", b, q, o)
    n = o.shape[0] - 1
    db, dq, do = torch.from_numpy(b).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(o.view(np.int64)).cuda()
    for w in range(4, MAX_W + 1):
        what = "declared-%s-%d w%d" % (geom, scores, w)
        di = torch.zeros(n, dtype=torch.int64, device="cuda")
        ds = torch.full((n,), float(np.finfo(np.float32).min), dtype=torch.float32, device="cuda") if scores else None
        m.counters(reset=True)
        m.match_unique(db, dq, do, info=di, score=ds, max_patl=32 * w)
        info = di.cpu().numpy().view(np.uint64)
        assert np.array_equal(info, oinfo), "%s: records: %s" % (what, _first_diff(info, oinfo))
        if scores:
            sb, ob = ds.cpu().numpy().view(np.uint32), oscore.view(np.uint32)
            assert np.array_equal(sb, ob), "%s: score bits: %s" % (what, _first_diff(sb, ob))
        _check_counters(m, octr, what)


# ---------------------------------------------------------------------------------------------------------------------
# 4. filter levels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,patl", [("rows", 100), ("starts", 150)], ids=["rows-w4", "starts-w5"])
def test_filter_levels(ora, geom, patl):
    """Reads with diverged near-copies (synth.diverged_copy_reads: the record depends on the order of the update() calls
    and on eps = filter_mult * patl) at filter levels 0 (eps = 0: the edge of the precondition of flush_pending's merge of
    repeated calls), 1, 3 and 4, scores on"""
    gm = GEOMETRIES[geom]
    g = synth.random_genome(400_000, seed=60_000 + patl, n_frag=3, n_runs=6)
    b = synth.diverged_copy_reads(g, 500, patl, gm.seedl, seed=60_001 + patl, q_max=63)
    og = ora.Genome(g.sym, g.frag_start)
    ix = ora.Index(og, gm.seedl)
    k = 5
    m = UniqueMatcher(RealOptions(seedl=gm.seedl, seedkmax=2, totalkmax=k).normalise(),
                      prefix_bits=gm.prefix_bits, table_kind=gm.table_kind)
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    assert m.table_kind == gm.layout, m.table_kind
    records = {}
    for level in (0, 1, 3, 4):
        m.set_match_params(seedkmax=2, totalkmax=k, scores=1, filter_level=level)
        p = ora.make_params(seedl=gm.seedl, seedkmax=2, totalkmax=k, scores=1, filter_level=level)
        oinfo, oscore, octr = ora.match_unique(og, ix, p, b.bases, b.qual, b.offsets)
        m.counters(reset=True)
        info, score = m.match_unique(b.bases, b.qual, patl=patl)
        what = "filter level %d" % level
        assert np.array_equal(info, oinfo), "%s: records: %s" % (what, _first_diff(info, oinfo))
        assert np.array_equal(score.view(np.uint32), oscore.view(np.uint32)), "%s: score bits" % what
        c = m.counters()
        for kk in WORK:
            assert c[kk] == octr[kk], (what, kk, c[kk], octr[kk])
        records[level] = oinfo
    st0, st4 = unpack_info(records[0])[0], unpack_info(records[4])[0]
    assert (st4 == NonUnique).sum() > (st0 == NonUnique).sum(), "the levels must decide records of this batch"
    m.close()
