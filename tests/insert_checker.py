"""Insert sizes restated in numpy -- TEST INFRASTRUCTURE ONLY: the outer distance of a pair record, the histogram of the
Unique records with its overflow bin and its invalid rule, and the quartile rule of real_hip_insert_bounds
(include/real_hip.h, "insert sizes").  Everything is done on Python integers or int64, never on uint32."""
from __future__ import annotations

import numpy as np

from pairs_checker import UNIQUE

MIN_COUNT = 32          # REAL_HIP_INSERT_MIN_COUNT
MAX_BINS = 16384        # REAL_HIP_INSERT_HIST_MAX_BINS
E_INVALID, E_OVERFLOW, E_STATE = -1, -4, -5


def outer_of(rec, len1, len2):
    """(outer distance as int64, valid) of every record as if it were Unique: the forward mate is mate 1 iff inverted1 == 0;
    outer = r.pos + len_r - f.pos; not valid: the forward mate starts behind the reverse one, or the reverse mate ends before
    the forward one starts"""
    p1, p2 = rec["pos1"].astype(np.int64), rec["pos2"].astype(np.int64)
    l1, l2 = np.asarray(len1).astype(np.int64), np.asarray(len2).astype(np.int64)
    fwd1 = rec["inverted1"] == 0
    fp, rp, lr = np.where(fwd1, p1, p2), np.where(fwd1, p2, p1), np.where(fwd1, l2, l1)
    outer = rp + lr - fp
    valid = (fp <= rp) & (rp + lr >= fp)
    return outer, valid


def histogram(rec, len1, len2, n_bins: int, hist=None):
    """-> (hist as uint64, stats): the counts are added to `hist` if one is given"""
    assert 2 <= n_bins <= MAX_BINS
    outer, valid = outer_of(rec, len1, len2)
    uniq = rec["state"] == UNIQUE
    take = uniq & valid
    bins = np.minimum(outer[take], n_bins - 1)
    h = np.bincount(bins, minlength=n_bins).astype(np.uint64)
    stats = {"records": int(rec.shape[0]), "counted": int(take.sum()), "overflow": int((outer[take] >= n_bins - 1).sum()),
             "invalid": int((uniq & ~valid).sum())}
    return (h if hist is None else hist + h), stats


def bounds(hist, min_count: int = MIN_COUNT, iqr_mult: int = 3):
    """the quartile rule on Python integers -> (status, dict): q_j = the smallest d with cum(d) >= (j n + 3) // 4"""
    h = [int(x) for x in hist]
    n = sum(h)
    est = {"n": n, "q1": 0, "median": 0, "q3": 0, "low": 0, "high": 0}
    if len(h) < 2:
        return E_INVALID, est
    if n < min_count or n == 0:
        return E_STATE, est
    q = []
    for j in (1, 2, 3):
        need, cum = (j * n + 3) // 4, 0
        for d, c in enumerate(h):
            cum += c
            if cum >= need:
                q.append(d)
                break
    est.update(q1=q[0], median=q[1], q3=q[2])
    if q[2] == len(h) - 1:
        return E_OVERFLOW, est
    reach = iqr_mult * (q[2] - q[0])
    est.update(low=q[0] - min(q[0], reach), high=min(0xffffffff, q[2] + reach))
    return 0, est
