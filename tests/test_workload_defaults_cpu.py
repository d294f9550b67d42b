"""The shared paired-end workloads with their default arguments are the inputs they have always been: the hashes below
were taken before search_workload / pair_workload learnt to take their geometry as arguments."""
import hashlib

import numpy as np
import pytest

import mate_search_workloads as mw
import pairs_workloads as pw


def _h(*arrs):
    m = hashlib.sha256()
    for a in arrs:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()[:16]


# (workload, kind, ragged): sha256 over (sym, frag_start), and over (bases, qual, offsets) of mate batch 1 and 2
RECORDED = {
    ("mw", "iid", False): ("72cee1397050f193", "794979e8f5ff4578", "d169117495a06266"),
    ("pw", "iid", False): ("4db0ca83316866a3", "4aebd2dbd1be8051", "ccd114a60e45d0cc"),
    ("mw", "iid", True): ("812ccc61963937fe", "6dae43c44fd42298", "d253afa959f38f66"),
    ("pw", "iid", True): ("4db0ca83316866a3", "773e7d16dd4a993b", "8adb128d0a8c442c"),
    ("mw", "families", False): ("34487d9404ef78f6", "1987886b30d2a236", "2eaa984e34c5737c"),
    ("pw", "families", False): ("0b1d48df98dd3d7c", "47cd8d53270cc554", "46dee694277d40f9"),
    ("mw", "families", True): ("49bebdfc005f7107", "a4b1871d7edb7e72", "8357bc1092c48177"),
    ("pw", "families", True): ("0b1d48df98dd3d7c", "4c425e57373569f7", "31b5e90e0e72c5e1"),
}


@pytest.mark.parametrize("key", sorted(RECORDED), ids=lambda k: "%s-%s-%s" % (k[0], k[1], "ragged" if k[2] else "uniform"))
def test_default_workloads_are_unchanged(key):
    which, kind, ragged = key
    g, b1, b2 = (mw.search_workload(kind, ragged)[:3] if which == "mw" else pw.pair_workload(kind, ragged))
    got = (_h(g.sym, g.frag_start), _h(b1.bases, b1.qual, b1.offsets), _h(b2.bases, b2.qual, b2.offsets))
    assert got == RECORDED[key]


def test_random_qualities_leave_bases_alone_and_planted_reads_fixed():
    g0, a1, a2, planted = mw.search_workload("iid", True)
    g1, b1, b2, planted1 = mw.search_workload("iid", True, random_qual=True)
    assert planted == planted1 and np.array_equal(g0.sym, g1.sym)
    for a, b in ((a1, b1), (a2, b2)):
        assert np.array_equal(a.bases, b.bases) and np.array_equal(a.offsets, b.offsets)
        assert b.qual.max() == 63 and b.qual.min() == 0 and np.unique(b.qual).size == 64
        for cat in planted.values():
            for i in cat:
                assert (b.qual[int(b.offsets[i]):int(b.offsets[i + 1])] == 35).all()
    _, c1, _ = pw.pair_workload("iid", False, random_qual=True)
    assert np.unique(c1.qual).size == 64
