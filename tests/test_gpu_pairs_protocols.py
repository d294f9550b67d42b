"""The paired-end surface end to end at real protocol shapes (mate_search_workloads.PROTOCOL_ROWS): 2 x 150 with 64-base
seeds on wide bucket rows and on the fingerprint directory, 2 x 250, 128 + 96, and a ragged batch of every read width;
random per-base qualities, scores on and off, both genome kinds.  The search against mate_search_checker, the join
against pairs_checker, the enumeration against pairs_all_checker: every field and both FP64 values bit for bit, the
counters and the offsets exactly.  The coverage conditions are counted on the checkers alone (and asserted without a
GPU in test_mate_search_cpu.py)."""
import numpy as np
import pytest

import mate_search_checker as mc
import mate_search_workloads as mw
import pairs_all_checker as pac
import pairs_checker as pc
import pairs_workloads as pw
from real_amd import lib as rlib
from real_amd.matcher import PairMatcher, RealOptions

pytestmark = pytest.mark.gpu

FL = 2
LAYOUT = {"starts": rlib.LAYOUT_STARTS, "fingerprint": rlib.LAYOUT_FINGERPRINT, "rows": rlib.LAYOUT_ROWS}
ROW_IDS = [r.name for r in mw.PROTOCOL_ROWS]


def _matcher(row, g, scores):
    m = PairMatcher(RealOptions(seedl=row.seedl, seedkmax=2, totalkmax=row.tk, scores=bool(scores), filter_level=FL).normalise(),
                    prefix_bits=row.pb, table_kind=row.tkind)
    m.set_text_symbols(0, g.sym, g.frag_start)
    m.build_index_block()
    assert m.table_kind == LAYOUT[row.layout], (row.name, m.table_kind)
    return m


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("kind", ["iid", "families"])
@pytest.mark.parametrize("row", mw.PROTOCOL_ROWS, ids=ROW_IDS)
def test_match_pairs_search_at_protocol_shapes(ora, row, kind, scores):
    g, b1, b2, _ = mw.protocol_search_workload(row, kind)
    f = mw.oracle_lists(ora, g, b1, b2, row.seedl, row.tk, scores, FL)
    args = (b1, b2, row.min_ins, row.max_ins, scores, ora.filter_mult(FL, row.tk), row.seedl, row.tk)
    off, _ = mc.check_pairs_search(ora, {0: g}, [f], *args, search=False)
    on, ctr = mc.check_pairs_search(ora, {0: g}, [f], *args)
    mw.assert_coverage(off, on, f, "%s %s" % (row.name, kind))
    n = b1.n_reads
    if kind == "families":                                          # the hit buffers of the paired call start at n + n / 4 + 1024 hits and must grow
        assert max(int(f[2][-1]), int(f[4][-1])) > n + n // 4 + 1024, (int(f[2][-1]), int(f[4][-1]))
    if row.ragged_patl:
        for b in (b1, b2):
            assert {(int(v) + 31) // 32 for v in mw.lens_of(b)} >= set(range(2, 11)), "every width in one batch"
    m = _matcher(row, g, scores)
    got = m.match_pairs(b1, b2, row.min_ins, row.max_ins, mate_search=True)
    pc.assert_records_equal(got, on, "search on %s %s" % (row.name, kind))
    st = m.mate_search_stats(reset=True)
    assert {k: st[k] for k in mc.COUNTERS} == ctr and st["fragments"] == n and st["launches"] == 1, (st, ctr)
    pc.assert_records_equal(m.match_pairs(b1, b2, row.min_ins, row.max_ins), off, "search off %s %s" % (row.name, kind))
    assert m.mate_search_stats()["fragments"] == 0
    m.close()


@pytest.mark.parametrize("scores", [1, 0])
@pytest.mark.parametrize("kind", ["iid", "families"])
@pytest.mark.parametrize("row", mw.PROTOCOL_ROWS, ids=ROW_IDS)
def test_join_and_enumeration_at_protocol_shapes(ora, row, kind, scores):
    g, b1, b2 = mw.protocol_pair_workload(row, kind)
    f, single = pw.oracle_pairs(ora, g, b1, b2, row.seedl, row.tk, scores, FL, want_single=True)
    _, h1, o1, h2, o2 = f
    l1, l2 = pw.lens_of(b1), pw.lens_of(b2)
    want = pc.check_pairs([f], l1, l2, row.min_ins, row.max_ins, scores, ora.filter_mult(FL, row.tk))
    cov = pw.coverage(want, single)
    print(row.name, kind, scores, cov)
    assert cov["nomatch"] and cov["unique"] and cov["nonunique"] and cov["fwd_first"] and cov["fwd_second"] and cov["rescued"] > 0, cov
    all_want, woff = pac.enumerate_pairs(h1, o1, l1, h2, o2, l2, row.min_ins, row.max_ins, 0)
    exp = pac.expected_stats(o1, o2, all_want)
    per = (woff[1:] - woff[:-1]).astype(np.int64)
    assert all_want.shape[0] > 500
    if kind == "families":
        assert (per >= 2).sum() >= 20 and exp["handed_over"] > 0, (int((per >= 2).sum()), exp)
    m = _matcher(row, g, scores)
    pc.assert_records_equal(m.match_pairs(b1, b2, row.min_ins, row.max_ins), want, "join %s %s" % (row.name, kind))
    st = m.pair_stats()
    prod = (o1[1:] - o1[:-1]).astype(np.int64) * (o2[1:] - o2[:-1]).astype(np.int64)
    assert st["pairs"] == b1.n_reads and st["products"] == int(prod.sum()) and st["handed_over"] == int((prod > 32).sum()), st
    m.pair_all_stats(reset=True)
    got, off = m.match_pairs_all(b1, b2, row.min_ins, row.max_ins, cap=all_want.shape[0])
    np.testing.assert_array_equal(off, woff)
    pac.assert_pair_hits_equal(got, all_want, "enumeration %s %s" % (row.name, kind))
    st = m.pair_all_stats()
    assert st["fragments"] == b1.n_reads and {k: st[k] for k in exp} == exp, (st, exp)
    m.close()
