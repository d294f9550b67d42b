"""Row addressing of the pair tables (real_amd/csrc/row_addr.h: rh_sig_rcform, rh_place_sig, rh_row_addr), restated
here and checked exhaustively at seedl 8 and 12, without a GPU:

  * (list, signature) -> (table, row, key group) is a bijection at every group width the planner allows (gbits 1..4);
  * the four paired lookups land where the design says: the row found with the forward list-k signature (k = 0, 1) holds,
    in the group with `which` set, the list 5-k entries the REVERSE strand asks for, and the row found with the reverse
    list-k signature holds the list 5-k entries the forward strand asks for; the two groups differ in the `which` bit only.

The restatement pins the design; the helper as the library compiles it (real_amd/csrc/row_addr.h, no HIP in it) is
checked the same way by ``host_selftest rowaddr``, at seedl 8 and 12 exhaustively and at 16, 24 and 32 -- the benchmark's
geometry -- on two million drawn seeds (test_row_addr_header).  tests/test_gpu_paired_rows.py then builds an index with
it and reads it through it."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("l", (8, 12, 16, 24, 32))
def test_row_addr_header(l):
    host = os.path.join(ROOT, "real_amd", "host")
    subprocess.check_call(["make", "-C", host, "host_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "host_selftest"), "rowaddr", str(l)], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0 and r.stdout.split()[0] == "ok", r.stdout


MIX32 = 0x9E3779B1
SEGS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))       # rh_list_segs


def rcform(sign, l):
    """the reverse complement of the l/2 bases of an l-bit signature"""
    out = np.zeros_like(sign)
    for i in range(l // 2):
        out |= (3 - ((sign >> np.uint64(2 * i)) & np.uint64(3))) << np.uint64(l - 2 - 2 * i)
    return out


def row_addr(la, sign, l, gbits):
    place = rcform(sign, l) if la > 3 else sign
    mixed = (place * np.uint64(MIX32)) & np.uint64((1 << l) - 1)
    if la in (2, 3):
        return np.full(sign.shape, la), mixed >> np.uint64(gbits), mixed & np.uint64((1 << gbits) - 1)
    h = gbits - 1
    which = np.uint64((1 if la > 3 else 0) << h)
    return np.full(sign.shape, 5 - la if la > 3 else la), mixed >> np.uint64(h), which | (mixed & np.uint64((1 << h) - 1))


@pytest.mark.parametrize("l", (8, 12))
@pytest.mark.parametrize("gbits", (1, 2, 3, 4))
def test_row_address_is_a_bijection(l, gbits):
    sign = np.arange(1 << l, dtype=np.uint64)
    pb = l - gbits
    seen = set()
    for la in range(6):
        t, row, grp = row_addr(la, sign, l, gbits)
        assert int(row.max()) < ((2 << pb) if la not in (2, 3) else (1 << pb)) and int(grp.max()) < (1 << gbits)
        keys = set(zip(t.tolist(), row.tolist(), grp.tolist()))
        assert len(keys) == sign.shape[0], "list %d: two signatures share a (row, group)" % la
        assert not (keys & seen), "list %d shares a (table, row, group) with another list" % la
        seen |= keys
    # four tables: two of 2^(pb+1) rows, two of 2^pb, 2^gbits groups each = six lists of 2^l signatures
    assert len(seen) == 6 << l
    assert {k[0] for k in seen} == {0, 1, 2, 3}


@pytest.mark.parametrize("l", (8, 12))
def test_paired_lookups_land_in_one_row(l):
    """every seed of l bases: segments m0..m3 forward, r_i = rc(m_{3-i}) reverse"""
    gbits, q = 3, l // 4                           # q bases per segment
    rng = np.random.default_rng(l)
    seeds = np.arange(1 << (2 * l), dtype=np.uint64) if l == 8 else rng.integers(0, 1 << (2 * l), size=200_000).astype(np.uint64)
    seg = [(seeds >> np.uint64(2 * q * (3 - i))) & np.uint64((1 << (2 * q)) - 1) for i in range(4)]
    rseg = [rcform(seg[3 - i], 2 * q) for i in range(4)]

    def sig(s, la):
        a, c = SEGS[la]
        return (s[a] << np.uint64(2 * q)) | s[c]

    half = np.uint64(1 << (gbits - 1))
    for k in (0, 1):
        for own, other in ((seg, rseg), (rseg, seg)):
            t0, r0, g0 = row_addr(k, sig(own, k), l, gbits)              # this strand's list k
            t1, r1, g1 = row_addr(5 - k, sig(other, 5 - k), l, gbits)    # the other strand's list 5 - k
            assert np.array_equal(t0, t1) and np.array_equal(r0, r1), "lists %d / %d: not the same row" % (k, 5 - k)
            assert np.array_equal(g0 | half, g1) and not (g0 & half).any()
