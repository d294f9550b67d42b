"""The Python wrappers take numpy arrays as they come: a strided view of the bases, the qualities, the offsets or the records
gives exactly what the contiguous array gives, for every entry point that reads a batch.  Nothing here knows what the right
records are (the stages have their checkers elsewhere); only public methods are used."""
import numpy as np
import pytest

import pairs_workloads as pw
from real_amd.matcher import PairMatcher, RealOptions

pytestmark = pytest.mark.gpu
N, PATL = 65, 50                   # one tile of 64 reads and one more


def _strided(a):
    """the values of `a` as every other element of an array twice as long: not contiguous"""
    v = np.repeat(a, 2)[::2]
    assert not v.flags.c_contiguous and v.tobytes() == np.ascontiguousarray(a).tobytes()
    return v


@pytest.fixture(scope="module")
def load():
    """a genome of 6000 bases with its index, 65 fragments with mates of 50 bases and qualities (mate 1: the 65 single reads)"""
    import torch
    torch.zeros(1, device="cuda")      # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    g, b1, b2 = pw.pair_workload("iid", False, patl=(PATL, PATL), n=N, size=6000)
    assert b1.n_reads == b2.n_reads == N and len(b1.bases) == N * PATL and b1.qual is not None
    m = PairMatcher(RealOptions(seedl=32, seedkmax=2, totalkmax=3, scores=True, filter_level=2).normalise())
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    plain = [(b.bases, b.qual, b.offsets) for b in (b1, b2)]
    views = [tuple(_strided(a) for a in mate) for mate in plain]
    yield m, plain, views, g.n
    m.close()


def _same(a, b):
    """two results: arrays (bytes and shape), or tuples of them"""
    if isinstance(a, tuple):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif a is None:
        assert b is None
    else:
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_matching_takes_strided_views(load):
    m, (r, r2), (v, v2), n_bases = load
    info, score = m.match_unique(*r)
    st = info >> np.uint64(61)
    assert ((st == 1) | (st == 2)).sum() > N // 8, "reads are placed (many lie in the genome's repeats)"
    _same(m.match_unique(*v), (info, score))
    _same(m.match_unique(v[0], v[1], patl=PATL), (info, score))                 # uniform length: no offsets
    hits = m.match_all(*r)
    assert hits[0].shape[0] > N
    _same(m.match_all(*v), hits)
    _same(m.match_all(*v, cap=1), hits)                                         # and through the grown list
    pairs = m.match_pairs(r, r2, pw.MIN_INS, pw.MAX_INS)
    assert (pairs["state"] == 1).sum() > N // 4, "fragments pair"
    _same(m.match_pairs(v, v2, pw.MIN_INS, pw.MAX_INS), pairs)
    _same(m.match_pairs(v, v2, pw.MIN_INS, pw.MAX_INS, mate_search=True), m.match_pairs(r, r2, pw.MIN_INS, pw.MAX_INS, mate_search=True))
    _same(m.match_pairs_singles(v, v2, pw.MIN_INS, pw.MAX_INS), m.match_pairs_singles(r, r2, pw.MIN_INS, pw.MAX_INS))
    _same(m.match_pairs_all(v, v2, pw.MIN_INS, pw.MAX_INS), m.match_pairs_all(r, r2, pw.MIN_INS, pw.MAX_INS))


def test_stages_take_strided_views_of_reads_and_records(load):
    m, (r, r2), (v, v2), n_bases = load
    info, _ = m.match_unique(*r)
    pairs, s1, s2 = m.match_pairs_singles(r, r2, pw.MIN_INS, pw.MAX_INS)
    vinfo, vpairs, vs1, vs2 = (_strided(a) for a in (info, pairs, s1, s2))

    def pileup_and_calls(reads, mate2, rec, prec):
        m.pileup_begin(0)
        m.pileup_add(reads[0], reads[1], rec, reads[2])
        m.pileup_add_pairs(reads, mate2, prec)
        n_sites = m.pileup_finish()
        sites, depth = m.pileup_sites(cap=4), m.pileup_depth(0, n_bases)
        assert n_sites == len(sites) > 4 and int(depth.max()) > 1
        m.call_begin()
        m.call_add(reads[0], reads[1], rec, reads[2])
        m.call_add_pairs(reads, mate2, prec)
        n_calls = m.call_finish(0, 0)
        out = (sites, depth, m.call_evidence(cap=4), m.call_variants(cap=1))
        assert n_calls == len(out[3]) and len(out[2]) == n_sites
        m.call_end()
        m.pileup_end()
        return out
    _same(pileup_and_calls(v, v2, vinfo, vpairs), pileup_and_calls(r, r2, info, pairs))

    lists = m.mismatches(r[0], r[1], info, r[2])
    assert len(lists[0]) > 4
    _same(m.mismatches(v[0], v[1], vinfo, v[2]), lists)
    _same(m.mismatches(v[0], v[1], vinfo, v[2], cap=1), lists)
    _same(m.mismatches_pairs(v, v2, vpairs), m.mismatches_pairs(r, r2, pairs))
    _same(m.mismatches_pairs(v, v2, vpairs, vs1, vs2, cap=1), m.mismatches_pairs(r, r2, pairs, s1, s2))
    sums = m.read_summary(*r)
    assert sums["len"].tolist() == [PATL] * N and sums["qsum"].max() > 0
    _same(m.read_summary(*v), sums)
    _same(m.mark_duplicates(vinfo, _strided(sums)), m.mark_duplicates(info, sums))
