"""What the insert-size tests share -- TEST INFRASTRUCTURE ONLY: the two whole-path workloads with the oracle's hit lists
(computed once per session) and the checker's pair records under a window."""
from __future__ import annotations

import functools

import insert_checker as ic
import pairs_checker as pc
import pairs_workloads as pw

WORKLOADS = [("iid", True), ("families", False)]
WINDOW = (0, 1000)                  # the defaults of -insert_min / -insert_max: the probe's window
SEEDL, TOTALK, FILTER_LEVEL = 32, 3, 2
SAMPLE = 200                        # fragments the CPU test takes the bounds from


@functools.lru_cache(maxsize=None)
def workload(kind: str, ragged: bool):
    return pw.pair_workload(kind, ragged)


_lists = {}


def oracle_lists(ora, kind: str, ragged: bool, scores: int):
    """(fileid, hits1, off1, hits2, off2) of the workload from the oracle's match_all"""
    key = (kind, ragged, int(scores))
    if key not in _lists:
        g, b1, b2 = workload(kind, ragged)
        _lists[key] = pw.oracle_pairs(ora, g, b1, b2, SEEDL, TOTALK, int(scores), FILTER_LEVEL)[0]
    return _lists[key]


def first_fragments(f, n: int):
    """the lists of the first n fragments"""
    fid, h1, o1, h2, o2 = f
    return fid, h1[:int(o1[n])], o1[:n + 1], h2[:int(o2[n])], o2[:n + 1]


def records(ora, kind: str, ragged: bool, scores: int, window=WINDOW, n=None):
    """the checker's records of the (first n) fragments under the window -> (records, len1, len2)"""
    g, b1, b2 = workload(kind, ragged)
    f = oracle_lists(ora, kind, ragged, scores)
    l1, l2 = pw.lens_of(b1), pw.lens_of(b2)
    if n is not None:
        f, l1, l2 = first_fragments(f, n), l1[:n], l2[:n]
    return pc.check_pairs([f], l1, l2, window[0], window[1], int(scores), ora.filter_mult(FILTER_LEVEL, TOTALK)), l1, l2


def sample_bounds(rec, l1, l2, window=WINDOW):
    """the bounds `real -insert_auto` takes from the records of a sample: (status, estimate, (a, b))"""
    hist, _ = ic.histogram(rec, l1, l2, window[1] + 2)
    rc, est = ic.bounds(hist, ic.MIN_COUNT, 3)
    return rc, est, (max(window[0], est["low"]), min(window[1], est["high"]))


def unique_outers(rec, l1, l2):
    outer, valid = ic.outer_of(rec, l1, l2)
    u = rec["state"] == pc.UNIQUE
    assert valid[u].all()
    return outer[u]


def records_with_search(ora, kind: str, ragged: bool, scores: int, n: int, window=WINDOW):
    """the records of the first n fragments with the mate search behind the join (mate_search_checker.py)"""
    import types

    import mate_search_checker as mc
    g, b1, b2 = workload(kind, ragged)
    f = first_fragments(oracle_lists(ora, kind, ragged, scores), n)
    s1, s2 = (types.SimpleNamespace(n_reads=n, bases=b.bases, qual=b.qual, offsets=b.offsets[:n + 1]) for b in (b1, b2))
    rec, _ = mc.check_pairs_search(ora, {0: g}, [f], s1, s2, window[0], window[1], int(scores), ora.filter_mult(FILTER_LEVEL, TOTALK), SEEDL, TOTALK)
    return rec, pw.lens_of(b1)[:n], pw.lens_of(b2)[:n]
