"""Row addressing with canonical tables for the self-conjugate lists 2 and 3 (real_amd/csrc/row_addr.h: rh_canon,
rh_row_addr), restated here and checked exhaustively at seedl 8 and 12 for the group widths the planner allows
(gbits 1..4), without a GPU:

  * per list, signature -> (row, key group) is a bijection, and the six lists are disjoint in (table, row, group);
  * a list-2 (list-3) signature and its rc-form land in ONE row and their groups differ in the `which` bit, bit gbits - 1,
    alone;
  * a signature that is its own rc-form has exactly one group (and no other signature shares it);
  * the d = N/2 class -- b = a + N/2, where "the smaller of d and N - d" does not tell the two orientations apart -- is
    paired like every other: one row, one index, `which` 0 and 1;
  * the forward and the reverse strand's list-2 (list-3) lookups of a seed land in one row (every seed at seedl 8, drawn
    ones at 12).

The restatement pins the design (the `la in (2, 3)` branch of tests/test_paired_rows_cpu.py describes the layout before
this one: a table of its own per list); the header as the library compiles it is checked the same way by
``host_selftest rowaddr`` (tests/test_paired_rows_cpu.py::test_row_addr_header), and tests/test_gpu_canonical_rows.py builds
an index with it and reads it through it."""
import numpy as np
import pytest

MIX32 = 0x9E3779B1
SEGS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))       # rh_list_segs
U = np.uint64


def rcform(sign, l):
    """the reverse complement of the l/2 bases of an l-bit signature"""
    out = np.zeros_like(sign)
    for i in range(l // 2):
        out |= (U(3) - ((sign >> U(2 * i)) & U(3))) << U(l - 2 - 2 * i)
    return out


def canon(sign, l):
    """(index of l - 1 bits, which, self) of a list-2 / list-3 signature, by cases as the design's table states them"""
    h2 = l // 2
    N, half = 1 << h2, 1 << (h2 - 1)
    a = (sign >> U(h2)).astype(np.int64)
    b = rcform(sign & U(N - 1), h2).astype(np.int64)
    d = (b - a) % N
    x = np.where(d == 0, half + a % half, np.where(d == half, np.minimum(a, b), np.where(d < half, a, b)))
    ds = np.where((d == 0) | (d == half), 0, np.where(d < half, d, N - d))
    which = np.where(d == 0, a >> (h2 - 1), np.where(d == half, a > b, d > half)).astype(np.int64)
    return ((x << (h2 - 1)) | ds).astype(np.uint64), which.astype(np.uint64), d == 0


def row_addr(la, sign, l, gbits):
    h = gbits - 1
    low = U((1 << h) - 1)
    if la in (2, 3):
        index, which, _ = canon(sign, l)
        mixed = (index * U(MIX32)) & U((1 << (l - 1)) - 1)
        return np.full(sign.shape, la), mixed >> U(h), (which << U(h)) | (mixed & low)
    place = rcform(sign, l) if la > 3 else sign
    mixed = (place * U(MIX32)) & U((1 << l) - 1)
    return np.full(sign.shape, 5 - la if la > 3 else la), mixed >> U(h), U((1 if la > 3 else 0) << h) | (mixed & low)


@pytest.mark.parametrize("l", (8, 12))
@pytest.mark.parametrize("gbits", (1, 2, 3, 4))
def test_bijection_and_disjoint_lists(l, gbits):
    sign = np.arange(1 << l, dtype=np.uint64)
    pb = l - gbits
    seen = set()
    for la in range(6):
        t, row, grp = row_addr(la, sign, l, gbits)
        assert int(row.max()) < ((1 << pb) if la in (2, 3) else (2 << pb)) and int(grp.max()) < (1 << gbits)
        keys = set(zip(t.tolist(), row.tolist(), grp.tolist()))
        assert len(keys) == sign.shape[0], "list %d: two signatures share a (row, group)" % la
        assert not (keys & seen), "list %d shares a (table, row, group) with another list" % la
        seen |= keys
    # two pair tables of 2^(pb+1) rows, two canonical tables of 2^pb, 2^gbits groups each = six lists of 2^l signatures:
    # every (table, row, group) is taken, so the mean load of a row is what it was
    assert len(seen) == 6 << l and {k[0] for k in seen} == {0, 1, 2, 3}


@pytest.mark.parametrize("l", (8, 12))
@pytest.mark.parametrize("gbits", (1, 2, 3, 4))
def test_signature_and_rcform_share_a_row(l, gbits):
    sign = np.arange(1 << l, dtype=np.uint64)
    rf = rcform(sign, l)
    assert np.array_equal(rcform(rf, l), sign)
    wbit = U(1 << (gbits - 1))
    selfrc = rf == sign
    assert int(selfrc.sum()) == 1 << (l // 2)      # a free high half, the low half follows
    for la in (2, 3):
        _, r0, g0 = row_addr(la, sign, l, gbits)
        _, r1, g1 = row_addr(la, rf, l, gbits)
        assert np.array_equal(r0, r1), "list %d: a signature and its rc-form in different rows" % la
        assert np.array_equal((g0 ^ g1)[~selfrc], np.full(int((~selfrc).sum()), wbit)), "groups differ in more than `which`"
        # its own rc-form: exactly one group (the bijection above says nobody else is in it)
        assert np.array_equal(g0[selfrc], g1[selfrc])
    index, which, self_ = canon(sign, l)
    ir, wr, _ = canon(rf, l)
    assert np.array_equal(self_, selfrc) and np.array_equal(index, ir) and int(index.max()) < (1 << (l - 1))
    assert np.array_equal((which ^ wr)[~selfrc], np.ones(int((~selfrc).sum()), dtype=np.uint64))
    # (index, which) names every signature once
    assert len(set(zip(index.tolist(), which.tolist()))) == 1 << l


@pytest.mark.parametrize("l", (8, 12))
def test_half_way_class_is_paired(l):
    """d = N/2: b = a + N/2 (mod N); the rc-form has d = N/2 too"""
    h2 = l // 2
    N, half = 1 << h2, 1 << (h2 - 1)
    a = np.arange(N, dtype=np.uint64)
    b = (a + U(half)) & U(N - 1)
    sign = (a << U(h2)) | rcform(b, h2)                       # low half = rc(b), so that rc(low half) = b
    rf = rcform(sign, l)
    assert np.array_equal(rf >> U(h2), b) and not (rf == sign).any()
    index, which, self_ = canon(sign, l)
    ir, wr, _ = canon(rf, l)
    assert not self_.any() and np.array_equal(index, ir)
    assert np.array_equal(index, np.minimum(a, b) << U(h2 - 1))            # slot 0 of min(a, b) < N/2
    assert np.array_equal(which, (a > b).astype(np.uint64)) and np.array_equal(which ^ wr, np.ones(N, dtype=np.uint64))
    # ... and the self-rc class takes slot 0 of the x >= N/2: the two classes do not meet
    s_index, _, s_self = canon((a << U(h2)) | rcform(a, h2), l)
    assert s_self.all() and not (set(s_index.tolist()) & set(index.tolist()))
    for gbits in (1, 2, 3, 4):
        for la in (2, 3):
            _, r0, g0 = row_addr(la, sign, l, gbits)
            _, r1, g1 = row_addr(la, rf, l, gbits)
            assert np.array_equal(r0, r1) and np.array_equal(g0 ^ g1, np.full(N, U(1 << (gbits - 1))))


@pytest.mark.parametrize("l", (8, 12))
def test_both_strands_lookups_land_in_one_row(l):
    """every seed of l bases (drawn ones at l = 12): segments m0..m3 forward, r_i = rc(m_{3-i}) reverse"""
    q = l // 4                                     # q bases per segment
    rng = np.random.default_rng(l)
    seeds = np.arange(1 << (2 * l), dtype=np.uint64) if l == 8 else rng.integers(0, 1 << (2 * l), size=200_000).astype(np.uint64)
    seg = [(seeds >> U(2 * q * (3 - i))) & U((1 << (2 * q)) - 1) for i in range(4)]
    rseg = [rcform(seg[3 - i], 2 * q) for i in range(4)]

    def sig(s, la):
        a, c = SEGS[la]
        return (s[a] << U(2 * q)) | s[c]

    for gbits in (1, 3, 4):
        wbit = U(1 << (gbits - 1))
        for k in (2, 3):
            sf, sr = sig(seg, k), sig(rseg, k)
            assert np.array_equal(sr, rcform(sf, l))
            _, r0, g0 = row_addr(k, sf, l, gbits)
            _, r1, g1 = row_addr(k, sr, l, gbits)
            assert np.array_equal(r0, r1), "list %d: the two strands read different rows" % k
            same = sf == sr
            assert np.array_equal(g0[same], g1[same]) and np.array_equal((g0 ^ g1)[~same], np.full(int((~same).sum()), wbit))
