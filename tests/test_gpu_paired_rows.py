"""Pair tables of the narrow bucket rows (real_hip_internal.h: paired bucket rows): lists 0 / 5 and 1 / 4 share a table, the
entries of lists 5 and 4 are placed by the rc-form of their signature.  Index and matches against the oracle at the group
widths the planner allows (gbits 3, 1 -- the group is the `which` bit alone -- and 4), on one genome of 300 kbp with

  * a 60-copy family (complex pair rows, the second pass and the wave matcher read the new format),
  * a region that is its own reverse complement (list-0 and list-5 entries of one window meet in one row),

and reads planted on both strands with 0..3 substitutions, placed so that each of the six lists is the only one that
finds some read (two of the four seed segments hit), reads whose seed is its own reverse complement (then (m0, m1) = (rc m3, rc m2) and (m0, m2) =
(rc m3, rc m1): the two lookups of either pair table are the same row), reads with N, reads shorter than the seed; batches of 1, 63, 65 and 130 reads.

32-base seeds are left out: the planner allows bucket rows there from prefix_bits 28 on only (about 200 GB of rows); the
benchmark's GPU == CPU check over its whole read set is their pin, as for tests/test_gpu_instances.py."""
import numpy as np
import pytest

from real_amd import host_index, synth
from real_amd.lib import LAYOUT_ROWS
from real_amd.matcher import RealOptions, UniqueMatcher

pytestmark = pytest.mark.gpu

GEOMETRIES = {"l16-pb13": (16, 13), "l16-pb15": (16, 15), "l24-pb20": (24, 20)}
WORK = ("reads", "lookups", "candidates", "seedpass", "hits")
PATL, SEG, COPIES = 80, 400, 60
_cache = {}


def _genome():
    if "g" not in _cache:
        g, fam = synth.repeat_family_genome(300_000, seed=4242, families=(3, COPIES), seg_len=SEG, n_frag=3, n_runs=4)
        rng = np.random.default_rng(99)
        x = rng.integers(0, 4, size=300, dtype=np.uint8)
        pal = 150_000
        g.sym[pal:pal + 600] = np.concatenate([x, synth.revcomp(x)])    # its own reverse complement, centre at pal + 300
        _cache["g"] = (g, fam, pal)
    return _cache["g"]


def _reads(seedl):
    """the batch of 130 reads for seed length seedl"""
    key = ("reads", seedl)
    if key in _cache:
        return _cache[key]
    g, fam, pal = _genome()
    rng = np.random.default_rng(1000 + seedl)
    q = seedl // 4
    out = []

    def locus(L=PATL):
        while True:
            p = int(rng.integers(0, g.n - L))
            r = g.sym[p:p + L].copy()
            if (r < 4).all():
                return r

    # each list alone: one substitution in either of the two segments the list is NOT keyed on, both strands
    for a, c in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
        for inv in (0, 1):
            r = locus()
            if inv:
                r = synth.revcomp(r)
            for sgm in set(range(4)) - {a, c}:
                i = sgm * q + int(rng.integers(q))
                r[i] = (r[i] + 1 + int(rng.integers(3))) & 3
            out.append(r)
    # 0..3 substitutions anywhere, both strands
    for i in range(60):
        r = locus()
        for j in rng.choice(PATL, size=i % 4, replace=False):
            r[j] = (r[j] + 1 + int(rng.integers(3))) & 3
        out.append(synth.revcomp(r) if i & 1 else r)
    # the seed is its own reverse complement: in the genome (the centre of the palindromic region) and nowhere
    out.append(g.sym[pal + 300 - seedl // 2:][:PATL].copy())
    out.append(synth.revcomp(g.sym[pal + 300 - seedl // 2:][:PATL]))
    h = rng.integers(0, 4, size=seedl // 2, dtype=np.uint8)
    out.append(np.concatenate([h, synth.revcomp(h), rng.integers(0, 4, size=PATL - seedl, dtype=np.uint8)]))
    # inside the palindromic region, off centre, both strands
    for d in (20, 130, 250):
        out.append(g.sym[pal + d:pal + d + PATL].copy())
        out.append(synth.revcomp(g.sym[pal + 500 - d:pal + 500 - d + PATL]))
    # the families: 3 copies (parked), 60 copies (second pass / wave matcher)
    for i in range(24):
        c = fam[i % 2][int(rng.integers(len(fam[i % 2])))]
        r = g.sym[c + int(rng.integers(0, SEG - PATL)):][:PATL].copy()
        if i % 3 == 0:
            r[int(rng.integers(PATL))] ^= 1
        out.append(synth.revcomp(r) if i & 2 else r)
    # N, shorter than the seed, random
    r = locus(); r[5] = 4; out.append(r)
    r = locus(); r[PATL - 1] = 4; out.append(r)
    out.append(locus(seedl - 1))
    out.append(locus(seedl - 3))
    while len(out) < 130:
        out.append(rng.integers(0, 4, size=PATL, dtype=np.uint8))
    assert len(out) == 130
    order = rng.permutation(130)
    out = [out[i] for i in order]
    bases = np.concatenate(out).astype(np.uint8)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in out])]).astype(np.uint64)
    qual = rng.integers(0, 64, size=bases.shape[0]).astype(np.uint8)
    _cache[key] = (bases, qual, offsets)
    return _cache[key]


def _ora(ora, seedl):
    key = ("ora", seedl)
    if key not in _cache:
        g, _, _ = _genome()
        og = ora.Genome(g.sym, g.frag_start)
        _cache[key] = (og, ora.Index(og, seedl))
    return _cache[key]


@pytest.fixture(scope="module")
def matchers():
    made = {}

    def get(geom):
        if geom not in made:
            seedl, pb = GEOMETRIES[geom]
            g, _, _ = _genome()
            m = UniqueMatcher(RealOptions(seedl=seedl, seedkmax=2, totalkmax=3).normalise(), prefix_bits=pb, table_kind=3)
            m.set_text_symbols(0, g.sym, g.frag_start)
            m.build_index_block()
            assert m.table_kind == LAYOUT_ROWS and m.prefix_bits == pb
            made[geom] = m
        return made[geom]

    yield get
    for m in made.values():
        m.close()


def _slice(bases, qual, offsets, n):
    e = int(offsets[n])
    return bases[:e], qual[:e], offsets[:n + 1]


@pytest.mark.parametrize("n", (1, 63, 65, 130))
@pytest.mark.parametrize("inst", ("unique-scores", "all", "unique-noscores"))
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_matches_equal_oracle(ora, matchers, geom, inst, n):
    seedl, _ = GEOMETRIES[geom]
    m = matchers(geom)
    scores = 0 if inst == "unique-noscores" else 1
    m.set_match_params(seedkmax=2, totalkmax=3, scores=scores, filter_level=2)
    b, q, o = _slice(*_reads(seedl), n)
    og, ix = _ora(ora, seedl)
    p = ora.make_params(seedl=seedl, seedkmax=2, totalkmax=3, scores=scores, filter_level=2)
    m.counters(reset=True)
    if inst == "all":
        ohits, ooff, octr = ora.match_all(og, ix, p, b, q, o)
        hits, hoff = m.match_all(b, q, o, cap=int(ohits.shape[0]) + 16)
        assert np.array_equal(hoff, ooff)
        for f in ("read", "pos", "frag", "k", "inverted"):
            assert np.array_equal(hits[f].astype(np.int64), ohits[f].astype(np.int64)), f
        assert np.array_equal(hits["score"].view(np.uint32), ohits["score"].view(np.uint32))
    else:
        oinfo, oscore, octr = ora.match_unique(og, ix, p, b, q, o)
        info, score = m.match_unique(b, q, o)
        assert np.array_equal(info, oinfo), "records: reads %s differ" % np.nonzero(info != oinfo)[0][:8]
        if scores:
            assert np.array_equal(score.view(np.uint32), oscore.view(np.uint32))
    c = m.counters()
    for kk in WORK:
        assert c[kk] == octr[kk], "work counter %s %d != oracle %d" % (kk, c[kk], octr[kk])
    if n == 130:    # the 60-copy family: its reads outgrow a lane of the first pass
        assert c["handed_over"] > 0


@pytest.mark.parametrize("geom", ("l16-pb15", "l24-pb20", "l16-pb13"))
def test_index_device_equals_host_equals_oracle(ora, matchers, geom):
    seedl, pb = GEOMETRIES[geom]
    g, _, _ = _genome()
    a = matchers(geom)
    h = UniqueMatcher(RealOptions(seedl=seedl, seedkmax=2, totalkmax=3).normalise(), prefix_bits=pb, table_kind=3)
    text, wild = host_index.pack_text(g.sym)
    h.set_text(0, text, wild, g.n, g.frag_start)
    sign, pos, n, _nxt = host_index.build_lists(g.sym, seedl)
    h.set_index_block(sign, pos)
    assert h.table_kind == LAYOUT_ROWS and a.n_entries == h.n_entries == n
    _og, oix = _ora(ora, seedl)
    for k in range(6):
        ea, ba = a.index_download(k)
        eh, bh = h.index_download(k)
        assert np.array_equal(ea, eh) and np.array_equal(ba, bh), "list %d: device-built != host-uploaded" % k
        sg, ps = a.index_export(k)
        assert np.array_equal(sg.astype(np.uint64), oix.sign(k)) and np.array_equal(ps, oix.pos(k)), "exported list %d != reference list" % k
        # download: the canonical order (rh_mix32 of the list's OWN signature), bucket starts per prefix_bits prefix
        mixed = (oix.sign(k).astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64((1 << seedl) - 1)
        order = np.argsort(mixed, kind="stable")
        assert np.array_equal(ea[:, 1], oix.pos(k)[order]), "list %d: downloaded order" % k
        want = np.searchsorted(mixed[order] >> np.uint64(seedl - pb), np.arange((1 << pb) + 1), side="left")
        assert np.array_equal(ba.astype(np.int64), want), "list %d: bucket starts" % k
    h.close()
