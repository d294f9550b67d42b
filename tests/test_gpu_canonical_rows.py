"""Canonical tables of the narrow bucket rows (real_amd/csrc/row_addr.h): the entries of the self-conjugate lists 2 (m0, m3)
and 3 (m1, m2) are placed by a canonical index that a signature shares with its rc-form, so one row answers the forward and
the reverse strand's lookup of the list and the paired driver reads six rows per read.  Index and matches against the
oracle at the group widths the planner allows (gbits 3, 1 -- the group is the `which` bit alone -- and 4), on one genome
of 300 kbp with several fragments, N runs, a 3-copy and a 60-copy family (canonical rows go complex; the second pass and
the wave matcher read the new format) and, per seed length, planted loci whose seed window

  * has a list-2 (list-3) signature that is its own rc-form, m0 = rc m3 (m1 = rc m2), the whole seed not being so:
    both strands ask for the SAME key group;
  * lies in the d = N/2 class of list 2 (list 3), in either orientation;
  * is its own reverse complement as a whole.

Reads on those loci come from both strands with 0..3 substitutions outside the two segments of the list (with one in each
of the other two segments only that list finds the read); further reads only list 2 or only list 3 can find, reads with a
self-rc list-2 (list-3) signature that occurs nowhere in the genome, reads with N, reads shorter than the seed; batches of
1, 63, 65 and 130 reads.

32-base seeds are left out as in tests/test_gpu_paired_rows.py: the planner allows bucket rows there from prefix_bits 28
on only; the benchmark's GPU == CPU check over its whole read set is their pin."""
import numpy as np
import pytest

from real_amd import host_index, synth
from real_amd.lib import LAYOUT_ROWS
from real_amd.matcher import RealOptions, UniqueMatcher

pytestmark = pytest.mark.gpu

GEOMETRIES = {"l16-pb13": (16, 13), "l16-pb15": (16, 15), "l24-pb20": (24, 20)}
WORK = ("reads", "lookups", "candidates", "seedpass", "hits")
PATL, SEG, COPIES = 80, 400, 60
KINDS = ("self2", "self3", "half2-lo", "half2-hi", "half3-lo", "half3-hi", "selfseed")
_cache = {}


def _code(bases):
    v = 0
    for b in bases:
        v = (v << 2) | int(b)
    return v


def _canon_which(a, b, h2):
    """(`which`, self) of a list-2 / list-3 signature with high half a and rc(low half) b (row_addr.h: rh_canon)"""
    N, half = 1 << h2, 1 << (h2 - 1)
    d = (b - a) % N
    if d == 0:
        return a >> (h2 - 1), True
    return int(d > half or (d == half and a > b)), False


def _seed_window(kind, q, rng):
    """a seed of 4 q bases of the given kind"""
    m = [rng.integers(0, 4, size=q, dtype=np.uint8) for _ in range(4)]
    if kind == "selfseed":
        h = np.concatenate(m[:2])
        return np.concatenate([h, synth.revcomp(h)])
    x, y = (0, 3) if kind.endswith("2") or "2-" in kind else (1, 2)
    if kind.startswith("self"):
        m[y] = synth.revcomp(m[x])
        # (the whole seed is not its own reverse complement: the other two segments are not each other's)
        o = [i for i in range(4) if i not in (x, y)]
        while np.array_equal(m[o[1]], synth.revcomp(m[o[0]])):
            m[o[1]] = rng.integers(0, 4, size=q, dtype=np.uint8)
    else:
        # d = N/2: rc(m_y) = m_x with the top bit of its code flipped = its first base ^ 2; lo: a < b, hi: a > b
        a = m[x].copy()
        a[0] = (a[0] & 1) | (2 if kind.endswith("hi") else 0)
        b = a.copy()
        b[0] ^= 2
        m[x], m[y] = a, synth.revcomp(b)
    return np.concatenate(m)


def _genome():
    if "g" not in _cache:
        g, fam = synth.repeat_family_genome(300_000, seed=777, families=(3, COPIES), seg_len=SEG, n_frag=3, n_runs=4)
        rng = np.random.default_rng(5)
        taken = [(p, p + SEG) for f in fam for p in f]
        cuts = [int(c) for c in g.frag_start[1:-1]]
        planted = {}
        p = 1000
        for seedl in (16, 24):
            for kind in KINDS:
                # a clean stretch: no N, no fragment cut, no family copy within PATL of the window on either side
                while True:
                    lo, hi = p - PATL, p + seedl + PATL
                    if (g.sym[lo:hi] < 4).all() and not any(lo <= c <= hi for c in cuts) and not any(s < hi and lo < e for s, e in taken):
                        break
                    p += 97
                g.sym[p:p + seedl] = _seed_window(kind, seedl // 4, rng)
                planted[(seedl, kind)] = p
                taken.append((lo, hi))
                p += 2003
        _cache["g"] = (g, fam, planted)
    return _cache["g"]


def _absent_selfrc(g, seedl, la, rng):
    """segments (m_x, m_y = rc m_x) of list la such that no window of the genome has that list-la signature (None: there is none)"""
    q = seedl // 4
    x, y = (0, 3) if la == 2 else (1, 2)
    n = g.sym.shape[0]
    ok = np.ones(n - q + 1, dtype=bool)
    code = np.zeros(n - q + 1, dtype=np.int64)
    for j in range(q):
        s = g.sym[j:n - q + 1 + j].astype(np.int64)
        ok &= s < 4
        code = (code << 2) | (s & 3)
    nw = n - seedl + 1
    cx, cy = code[x * q:x * q + nw], code[y * q:y * q + nw]
    have = set(((cx << (2 * q)) | cy)[ok[x * q:x * q + nw] & ok[y * q:y * q + nw]].tolist())
    for _ in range(4096):
        mx = rng.integers(0, 4, size=q, dtype=np.uint8)
        my = synth.revcomp(mx)
        if ((_code(mx) << (2 * q)) | _code(my)) not in have:
            return mx, my
    return None


def _reads(seedl):
    """the batch of 130 reads for seed length seedl"""
    key = ("reads", seedl)
    if key in _cache:
        return _cache[key]
    g, fam, planted = _genome()
    rng = np.random.default_rng(2000 + seedl)
    q = seedl // 4
    out = []

    def locus(L=PATL):
        while True:
            p = int(rng.integers(0, g.n - L))
            r = g.sym[p:p + L].copy()
            if (r < 4).all():
                return r

    def sub(r, i):
        r[i] = (r[i] + 1 + int(rng.integers(3))) & 3

    # the planted loci, both strands: forward reads with 0 and 2 substitutions, reverse reads with 1 and 3
    for kind in KINDS:
        p = planted[(seedl, kind)]
        free = [0, 1, 2, 3] if kind == "selfseed" else [1, 2] if "2" in kind else [0, 3]    # segments the list is not keyed on
        for inv, nsub in ((0, 0), (0, 2), (1, 1), (1, 3)):
            # forward: the window is the read's seed; reverse: the read's seed is the reverse complement of the window
            w = g.sym[p:p + PATL].copy() if not inv else g.sym[p + seedl - PATL:p + seedl].copy()
            off = 0 if not inv else PATL - seedl
            assert (w < 4).all()
            if kind == "selfseed":
                for j in rng.choice(PATL - seedl, size=nsub, replace=False):
                    sub(w, (seedl if not inv else 0) + int(j))
            else:
                if nsub >= 1:
                    sub(w, off + free[0] * q + int(rng.integers(q)))
                if nsub >= 2:
                    sub(w, off + free[1] * q + int(rng.integers(q)))
                if nsub >= 3:
                    sub(w, (seedl if not inv else 0) + int(rng.integers(PATL - seedl)))
            out.append(synth.revcomp(w) if inv else w)
    # list 2 alone, list 3 alone: one substitution in either of the two segments the list is NOT keyed on, both strands
    for a, c in ((0, 3), (1, 2)):
        for inv in (0, 1):
            r = locus()
            if inv:
                r = synth.revcomp(r)
            for sgm in set(range(4)) - {a, c}:
                sub(r, sgm * q + int(rng.integers(q)))
            out.append(r)
    # a self-rc list-2 (list-3) signature that occurs nowhere
    for la in (2, 3):
        found = _absent_selfrc(g, seedl, la, rng)
        if found is not None:
            r = rng.integers(0, 4, size=PATL, dtype=np.uint8)
            x, y = (0, 3) if la == 2 else (1, 2)
            r[x * q:(x + 1) * q], r[y * q:(y + 1) * q] = found
            out.append(r)
    # 0..3 substitutions anywhere, both strands
    for i in range(32):
        r = locus()
        for j in rng.choice(PATL, size=i % 4, replace=False):
            sub(r, int(j))
        out.append(synth.revcomp(r) if i & 1 else r)
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


@pytest.mark.parametrize("seedl", (16, 24))
def test_batch_holds_the_cases(seedl):
    """(no device work: the batch is what the docstring says) both `which` values, self-rc signatures and the d = N/2 class of
    either orientation occur among the forward list-2 and list-3 signatures of the reads"""
    bases, _, offsets = _reads(seedl)
    q = seedl // 4
    h2 = 2 * q
    for x, y in ((0, 3), (1, 2)):
        which, selfs, halfway = set(), 0, set()
        for i in range(130):
            r = bases[int(offsets[i]):int(offsets[i + 1])]
            if r.shape[0] < seedl or (r[:seedl] > 3).any():
                continue
            a, b = _code(r[x * q:(x + 1) * q]), _code(synth.revcomp(r[y * q:(y + 1) * q]))
            w, s = _canon_which(a, b, h2)
            selfs += s
            if not s:
                which.add(w)
            if (b - a) % (1 << h2) == 1 << (h2 - 1):
                halfway.add(w)
        assert which == {0, 1} and selfs >= 4 and halfway == {0, 1}


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
        # download: the order of rh_mix32 of the list's OWN signature, bucket starts per prefix_bits prefix
        mixed = (oix.sign(k).astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64((1 << seedl) - 1)
        order = np.argsort(mixed, kind="stable")
        assert np.array_equal(ea[:, 1], oix.pos(k)[order]), "list %d: downloaded order" % k
        want = np.searchsorted(mixed[order] >> np.uint64(seedl - pb), np.arange((1 << pb) + 1), side="left")
        assert np.array_equal(ba.astype(np.int64), want), "list %d: bucket starts" % k
    h.close()
