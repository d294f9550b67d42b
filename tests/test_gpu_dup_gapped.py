"""The joint duplicate marking on the device (real_hip_mark_duplicates_gapped) against dup_gapped_checker.py, bit for bit, with
real_hip_dup_stats_get's counts: hand-made arrays around the wave and the block, every state of both records, the edges of the
key, host and device arrays; the records match_unique / match_gapped leave for the single-end workload (asserted to be the
oracle's / the checker's first); the identity with real_hip_mark_duplicates; every refusal, with nothing launched."""
import numpy as np
import pytest

import dup_checker as dk
import dup_gapped_checker as dgk
import gap_anchor_checker as gac
import gap_checker as gc
import single_gapped_workloads as sw
from real_amd import lib as rlib
from real_amd.matcher import AllMatcher, RealOptions, UniqueMatcher

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bare():
    """a context without text or index: the marking needs neither"""
    import torch
    torch.zeros(1, device="cuda")      # (a module fixture is set up before conftest's per-test one: PyTorch's runtime first, as there)
    m = UniqueMatcher(RealOptions(seedl=32, seedkmax=1, totalkmax=1, scores=False, filter_level=0).normalise())
    yield m
    m.close()


def _dev(a):
    import torch
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_sums(s):
    return _dev(s.view(np.int32).reshape(-1, 2))


def _dev_gaps(g):
    return _dev(np.ascontiguousarray(g).view(np.uint8).reshape(-1, 16))


def _lib_gaps(g):
    out = np.zeros(g.shape[0], dtype=rlib.GAP_PLACE_DTYPE)
    for k in gc.REC_DTYPE.names:
        out[k] = g[k]
    return out


def _mark(m, info, gaps, sums, on_device, want=None):
    """one marking call and its statistics against the checker's two formulations"""
    if want is None:
        want = dgk.mark_groups(info, gaps, sums)[:2]
        other = dgk.mark_sorted(info, gaps, sums)
        assert np.array_equal(want[0], other[0]) and want[1] == other[1]
    gaps = _lib_gaps(gaps)
    m.dup_stats(reset=True)
    if on_device:
        dup = m.mark_duplicates_gapped(_dev(info), _dev_gaps(gaps), _dev_sums(sums)).cpu().numpy()
    else:
        dup = m.mark_duplicates_gapped(info, gaps, sums)
    st = m.dup_stats(reset=True)
    assert dup.dtype == np.uint8 and np.array_equal(dup, want[0]), np.nonzero(dup != want[0])[0][:10]
    assert {k: st[k] for k in dk.STATS} == want[1], (st, want[1])
    assert st["launches"] == (3 if info.shape[0] else 0) and (st["kernel_ms"] > 0 or not info.shape[0])
    return dup


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("n", sw.HAND_N)
def test_marks_of_hand_made_arrays(bare, n, on_device):
    info, gaps, sums = sw.hand(n)
    if n >= 255:                       # the domain is there: every state of both records, both strands, every gap, length and file id
        kind = dgk.placements(info, gaps, sums)[0]
        assert {int(x) >> 61 for x in info} == {0, 1, 2, 3, 4} and {(int(t) >> 5) & 3 for t in gaps["tag"]} == {0, 1, 2, 3}
        assert set(gaps["gap"].tolist()) == set(sw.HAND_GAPS) and set(sums["len"].tolist()) == set(sw.HAND_LENGTHS)
        assert set(gaps["fileid"].tolist()) == set(sw.HAND_FILES) and {(int(t) >> 4) & 1 for t in gaps["tag"][kind == dgk.GAPPED]} == {0, 1}
        assert any(u and g for u, g in dgk.group_kinds(info, gaps, sums).values()) and (sums["qsum"] > sw.Q_TOP).any()
    _mark(bare, info, gaps, sums, on_device)


@pytest.mark.parametrize("on_device", [0, 1])
def test_the_edges_of_the_key(bare, on_device):
    """END5 beyond 2^32 and below 0, the info word that wins, the states that place nothing, file id 63, ties, the clamped qsum"""
    info, gaps, sums, want = sw.hand_edges()
    dup = _mark(bare, info, gaps, sums, on_device)
    assert dup.tolist() == want.tolist()
    # a file id beyond 63 in a gap record counts modulo 64: 64 + 1 meets 1
    g2 = gaps.copy()
    g2["fileid"][10] = 65
    assert _mark(bare, info, g2, sums, on_device).tolist() == want.tolist()
    assert dgk.keys(info, g2, sums)[10] == dgk.keys(info, gaps, sums)[10]


def test_a_group_of_300_of_both_kinds(bare):
    n = 300
    rng = np.random.default_rng(12)
    info = np.zeros(n, dtype=np.uint64)
    gaps = gc.empty_records(n)
    sums = np.zeros(n, dtype=dk.SUM_DTYPE)
    sums["len"], sums["qsum"] = 100, rng.integers(3000, 3010, size=n)
    for i in range(n):
        g = sw.HAND_GAPS[i % 5]
        if i % 2:
            info[i] = sw.info_word(2, 9000 - 100 + 1)
        else:
            gaps[i]["pos"], gaps[i]["gap"], gaps[i]["tag"], gaps[i]["split"] = 9000 - 100 - g + 1, g, dgk.gap_tag(gc.UNIQUE, 1), 1 if g else 0
    dup, st, groups = dgk.mark_groups(info, gaps, sums)
    assert st["groups"] == 1 and st["duplicates"] == n - 1 and (sums["qsum"] == sums["qsum"].max()).sum() > 10
    for on_device in (0, 1):
        _mark(bare, info, gaps, sums, on_device, (dup, st))


@pytest.mark.parametrize("on_device", [0, 1])
def test_no_unique_gap_record_is_todays_marking(bare, on_device):
    """all gap records NoMatch, and all NonUnique: dup[] and the statistics of real_hip_mark_duplicates"""
    info, gaps, sums = sw.hand(4099)
    for state in (gc.NOMATCH, gc.NONUNIQUE):
        g = gaps.copy()
        g["tag"] = (g["tag"] & ~np.uint8(3 << 5)) | np.uint8(state << 5)
        if state == gc.NOMATCH:
            g = gc.empty_records(g.shape[0])
        want = dk.mark_single(info, sums)
        bare.dup_stats(reset=True)
        plain = bare.mark_duplicates(_dev(info), _dev_sums(sums)).cpu().numpy() if on_device else bare.mark_duplicates(info, sums)
        st_plain = bare.dup_stats(reset=True)
        joint = _mark(bare, info, g, sums, on_device, want[:2])
        assert np.array_equal(plain, joint) and np.array_equal(plain, want[0])
        assert {k: st_plain[k] for k in dk.STATS} == want[1]


@pytest.mark.parametrize("on_device", [0, 1])
def test_marks_of_the_workload(ora, on_device):
    """match_unique and match_gapped on the device, their records asserted to be the oracle's and the checker's; then the marks"""
    w = sw.workload()
    info_w, gaps_w, sums_w, dup_w, st_w, _ = sw.expected(ora)
    m = AllMatcher(RealOptions(seedl=sw.SEEDL, seedkmax=sw.SEEDKMAX, totalkmax=sw.TOTALKMAX, scores=False, filter_level=0).normalise())
    try:
        m.set_text_symbols(0, w.g.sym, w.g.frag_start)
        m.build_index_block()
        info, _ = m.match_unique(w.b.bases, w.b.qual, offsets=w.b.offsets)
        assert np.array_equal(info, info_w)
        gaps = m.match_gapped(w.b, sw.AP.anchor_len, info=info, max_anchors=sw.AP.max_anchors, **w.prm._asdict())
        gac.assert_records_equal(gaps, gaps_w, "match_gapped")
        sums = m.read_summary(w.b.bases, w.b.qual, offsets=w.b.offsets, min_qual=sw.MIN_QUAL)
        assert np.array_equal(sums["len"], sums_w["len"]) and np.array_equal(sums["qsum"], sums_w["qsum"])
        m.dup_stats(reset=True)
        dup = _mark(m, info, gaps_w, sums_w, on_device, (dup_w, st_w))
        kind = dgk.placements(info_w, gaps_w, sums_w)[0]
        assert int(dup[kind == dgk.GAPPED].sum()) >= 50 and int(dup[kind == dgk.UNGAPPED].sum()) >= 50
        plain = dk.mark_single(info_w, sums_w)[0]
        assert not np.array_equal(plain, dup) and (plain[kind == dgk.UNGAPPED] != dup[kind == dgk.UNGAPPED]).any()   # (a gapped original outranks its cut copy)
    finally:
        m.close()


def test_errors_are_loud_and_launch_nothing(bare):
    import torch
    m = bare
    info, gaps, sums = sw.hand(64)
    gaps = _lib_gaps(gaps)
    dup = np.zeros(64, dtype=np.uint8)
    L, h, n = m._L, m._h, 64
    m.dup_stats(reset=True)

    def refused(word, rc):
        with pytest.raises(rlib.RealHipError, match=word) as e:
            m._check(rc)
        assert e.value.status == rlib.REAL_HIP_E_INVALID
        st = m.dup_stats()
        assert st["launches"] == 0 and st["reads"] == 0, word

    p = [info.ctypes.data, gaps.ctypes.data, sums.ctypes.data, n, 0, dup.ctypes.data]
    for k in (0, 1, 2, 5):
        q = list(p)
        q[k] = None
        refused("null", L.real_hip_mark_duplicates_gapped(h, *q))
    q = list(p)
    q[3] = (1 << 32) + 1                       # refused on the count alone (no array is looked at)
    refused("more than 2\\^32", L.real_hip_mark_duplicates_gapped(h, *q))
    # device arrays: info and summaries 8-byte, gap records 16-byte aligned
    room = torch.zeros(n * 16 + 64, dtype=torch.uint8, device="cuda")
    d_info, d_gaps, d_sums, d_dup = _dev(info), _dev_gaps(gaps), _dev_sums(sums), torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert room.data_ptr() % 16 == 0
    d = [d_info.data_ptr(), d_gaps.data_ptr(), d_sums.data_ptr(), n, 1, d_dup.data_ptr()]
    for k, shift, word in ((0, 4, "8-byte"), (2, 4, "8-byte"), (1, 8, "16-byte"), (1, 4, "16-byte")):
        q = list(d)
        q[k] = room.data_ptr() + shift
        refused(word, L.real_hip_mark_duplicates_gapped(h, *q))
    assert not d_dup.any().item() and not dup.any()
    # n == 0 with null arrays is valid, host and device
    assert L.real_hip_mark_duplicates_gapped(h, None, None, None, 0, 0, None) == 0 and L.real_hip_mark_duplicates_gapped(h, None, None, None, 0, 1, None) == 0
    with pytest.raises(ValueError, match="one side"):
        m.mark_duplicates_gapped(info, d_gaps, sums)
    with pytest.raises(ValueError, match="one gap record per info word"):
        m.mark_duplicates_gapped(info, gaps[:10], sums)
    assert m.dup_stats()["launches"] == 0
