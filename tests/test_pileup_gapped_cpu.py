"""Gapped placements in the pileup and the calls, the parts that need no GPU: the checker's two formulations against each other on
the hand-made records and on the gap checker's records over the CPU oracle's lists, the alt increments against the gapped
mismatch lists, g == 0 against the ungapped pileup, the depth identity, the indel calls that do not move, the coverage floors of
what the GPU tests run, and the exports, the header block and the mirror."""
import ctypes as C
import os

import numpy as np
import pytest

from abi_header import header_structs
import call_checker as ck
import gap_checker as gc
import gap_workloads as gw
import gapped_list_checker as glc
import gapped_list_workloads as glw
import indel_checker as ic
import indel_workloads as iw
import pileup_checker as pk
import pileup_gapped_checker as pgc
import pileup_gapped_workloads as pgw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 5
_CACHE = {}


def _gap_workload(ora):
    if "gw" not in _CACHE:
        w = glw.workload()
        pairs, s1, s2, _ = gw.oracle_records(ora, w)
        rec, _ = gc.check_gap(gc.Text(w["g"].sym, w["g"].frag_start, w["fileid"]), w["b1"], w["b2"], pairs, s1, s2, w["min_ins"], w["max_ins"], w["prm"])
        _CACHE["gw"] = (w["g"].sym, w["g"].frag_start, w["b1"], w["b2"], pairs, rec)
    return _CACHE["gw"]


def _planted(ora):
    if "pl" not in _CACHE:
        w = iw.planted()
        pairs, s1, s2, _ = iw.oracle_records(ora, w)
        rec, _ = gc.check_gap(gc.Text(w.g.sym, w.g.frag_start, 0), w.b1, w.b2, pairs, s1, s2, w.min_ins, w.max_ins, w.prm)
        _CACHE["pl"] = (w.g.sym, w.g.frag_start, w.b1, w.b2, pairs, rec)
    return _CACHE["pl"]


def _both(sym, b1, b2, gaps, min_qual, pairs=None, pb=None):
    """the pileup and the calls under both formulations, asserted equal -> (pileup, calls) of the first"""
    out = []
    for aligned in (pgc.aligned_by_pairs, pgc.aligned_by_diagonals):
        pu = pgc.GappedPileup(sym, 0, min_qual, aligned)
        if pairs is not None:
            pu.add_pairs(*(pb or (b1, b2)), pairs)
        pu.add_gapped(b1, b2, gaps)
        cl = pgc.GappedCalls(pu, aligned)
        if pairs is not None:
            cl.add_pairs(*(pb or (b1, b2)), pairs)
        cl.add_gapped(b1, b2, gaps)
        out.append((pu, cl))
    (pa, ca), (pb_, cb) = out
    assert np.array_equal(pa.depth, pb_.depth) and np.array_equal(pa.gdepth, pb_.gdepth) and np.array_equal(pa.alt, pb_.alt)
    assert pa.gstats == pb_.gstats and pa.stats == pb_.stats
    assert np.array_equal(ca.cnt, cb.cnt) and np.array_equal(ca.qsum, cb.qsum) and ca.gstats == cb.gstats and ca.stats == cb.stats
    return pa, ca


def _invariants(pu, cl):
    # the sum of depth[] equals bases + aligned_bases; gdepth is the gapped share
    assert int(pu.depth.sum()) == pu.stats["bases"] + pu.gstats["aligned_bases"]
    assert int(pu.gdepth.sum()) == pu.gstats["aligned_bases"] and (pu.gdepth <= pu.depth).all()
    assert int(pu.alt.sum()) == pu.stats["mismatches"] + pu.gstats["mismatches"]
    # cnt[s][b] == site.alt[b] for b != ref when the same records went to both
    sites = pu.sites()
    for b in range(4):
        sel = sites["ref"] != b
        assert np.array_equal(cl.cnt[sel, b], sites["alt"][sel, b])
    assert cl.stats["site_bases"] + cl.gstats["site_bases"] == int(cl.cnt.sum())


@pytest.mark.parametrize("min_qual", [0, 20])
def test_the_two_formulations_agree_on_the_hand_made_records(min_qual):
    for h in (glw.hand_cases(), pgw.hand_cases()):
        pu, cl = _both(h["sym"], h["b1"], h["b2"], h["gaps"], min_qual, h.get("pairs"), (h["pb1"], h["pb2"]) if "pairs" in h else None)
        _invariants(pu, cl)
        st = pu.gstats
        want = {"other_file": 0, "invalid": 0}
        for note in h["what"]:
            if pgw.EMPTY_NOTES.get(note):
                want[pgw.EMPTY_NOTES[note]] += 1
        assert (st["other_file"], st["invalid"]) == (want["other_file"], want["invalid"]) and st["invalid"] >= 11, st
        assert st["deleted"] > 0 and st["inserted"] > 0 and st["ungapped"] > 0 and st["n_dropped"] > 0
        assert (st["low_qual"] > 0) == (min_qual == 20 and "pairs" in h)                    # (gapped_list_workloads: every quality is 35)


def test_what_the_hand_made_set_holds():
    h = pgw.hand_cases()
    rec, n = h["gaps"], h["sym"].shape[0]
    bs = (h["b1"], h["b2"])
    lens = np.array([int(bs[int(gc.target_of(r["tag"]))].offsets[i + 1] - bs[int(gc.target_of(r["tag"]))].offsets[i]) for i, r in enumerate(rec)])
    placed = np.array([gc.state_of(r["tag"]) == gc.UNIQUE and int(r["fileid"]) == 0 and glc.fits(r, int(l), n) for r, l in zip(rec, lens)])
    assert n % 32 and n % 64 and 100_000 <= n <= 200_000
    assert set(lens[placed]) == set(pgw.LENGTHS) | {100} and set(rec["gap"][placed]) >= set(pgw.GAPS)
    pos = rec["pos"].astype(np.int64)
    for l in pgw.LENGTHS:
        for g in pgw.GAPS:
            sel = placed & (lens == l) & (rec["gap"] == g)
            assert set(rec["split"][sel]) >= set(pgw.splits_of(l, g)), (l, g)
            assert {0, 31} <= set(pos[sel] % 32), (l, g)
    assert {(int(gc.target_of(t)), int(gc.inverted_of(t))) for t in rec["tag"][placed]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert (pos[placed] == 0).any() and (pos[placed] + lens[placed] + rec["gap"][placed] == n).any()
    x = pos + rec["split"]
    across = placed & (rec["gap"] > 1) & (x // 32 != (x + rec["gap"] - 1) // 32)
    assert int(across.sum()) >= 16
    assert (h["b1"].qual < 20).any() and (h["b1"].qual >= 20).any()
    for note in pgw.EMPTY_NOTES:
        assert note in h["what"], note
    # N bits on deleted and on aligned positions of placed records
    is_n = h["sym"] > 3
    on_del = on_al = 0
    for i in np.nonzero(placed)[0]:
        g, j, p = int(rec["gap"][i]), int(rec["split"][i]), int(pos[i])
        on_del += bool(g > 0 and is_n[p + j:p + j + g].any())
        on_al += bool(is_n[pgc.aligned_by_diagonals(int(lens[i]), p, g, j)[1]].any())
    assert on_del >= 4 and on_al >= 20


def test_the_two_formulations_agree_on_the_oracles_records_and_the_floors_hold(ora):
    for name, (sym, frag_start, b1, b2, pairs, rec) in (("gap workload", _gap_workload(ora)), ("planted", _planted(ora))):
        pu, cl = _both(sym, b1, b2, rec, 20, pairs)
        _invariants(pu, cl)
        print(name, pu.gstats, cl.gstats)
        assert pu.gstats["invalid"] == 0 and pu.gstats["other_file"] == 0
        uniq = gc.state_of(rec["tag"]) == gc.UNIQUE
        tm, inv = gc.target_of(rec["tag"]), gc.inverted_of(rec["tag"])
        x = rec["pos"].astype(np.int64) + rec["split"]
        g = rec["gap"].astype(np.int64)
        gapped = uniq & (g != 0)
        straddle = gapped & np.where(g > 0, x // 32 != (x + g - 1) // 32, x % 32 != 0)   # a deletion across a word; a split inside one
        # a site of the finished pileup under the second segment
        is_site = pu.alt.sum(axis=1) > 0
        under = 0
        for i in np.nonzero(gapped)[0]:
            b = (b1, b2)[int(tm[i])]
            l = int(b.offsets[i + 1]) - int(b.offsets[i])
            ro, xs = pgc.aligned_by_diagonals(l, int(rec["pos"][i]), int(g[i]), int(rec["split"][i]))
            under += bool(is_site[xs[ro >= int(rec["split"][i]) + max(-int(g[i]), 0)]].any())
        classes = {"deletion": uniq & (g > 0), "insertion": uniq & (g < 0), "forward": gapped & (inv == 0), "reverse": gapped & (inv == 1),
                   "target mate 1": gapped & (tm == 0), "target mate 2": gapped & (tm == 1), "straddles a text word": straddle}
        for what, sel in classes.items():
            assert int(sel.sum()) >= FLOOR, (name, what, int(sel.sum()))
        assert under >= FLOOR, (name, under)


def test_alt_increments_are_the_gapped_lists_aligned_entries_filtered_by_quality():
    for h in (glw.hand_cases(), pgw.hand_cases()):
        sym, b1, b2, gaps = h["sym"], h["b1"], h["b2"], h["gaps"]
        lists, off, _ = glc.gapped_lists(sym, 0, b1, b2, gaps)
        for min_qual in (0, 20):
            pu = pgc.GappedPileup(sym, 0, min_qual)
            k = 0
            for i, read, qual, p, g, j, inv in pgc._records(pu, b1, b2, gaps):
                pu.place_gapped(read, qual, p, g, j, inv)
                xs, bases = pu.increments[k]
                k += 1
                L = lists[int(off[i]):int(off[i + 1])]
                L = L[(L["base"] != glc.DELETED) & (L["ref"] != 4)]                  # aligned, not on an N
                _, q = pgc._oriented(read, qual, inv)
                d = max(-g, 0)
                t = L["off"].astype(np.int64)
                ro = np.where(t < j, t, t - g) if g else t                          # the oriented read offset of text offset t
                assert not ((ro >= j) & (ro < j + d)).any()
                keep = q[ro] >= min_qual
                assert np.array_equal(xs, p + t[keep]) and np.array_equal(bases, L["base"][keep].astype(np.int64)), h["what"][i]
            assert k == pu.gstats["placed"] > 100


def test_an_ungapped_record_is_the_ungapped_placement():
    h = pgw.hand_cases()
    seen = 0
    for min_qual in (0, 20):
        a, b = pgc.GappedPileup(h["sym"], 0, min_qual), pk.Pileup(h["sym"], 0, min_qual)
        for i, read, qual, p, g, j, inv in pgc._records(a, h["b1"], h["b2"], h["gaps"]):
            if g == 0:
                a.place_gapped(read, qual, p, g, j, inv)
                b.place(read, qual, p, inv)
                seen += 1
        assert np.array_equal(a.depth, b.depth) and np.array_equal(a.alt, b.alt) and np.array_equal(a.gdepth, b.depth)
        assert (a.gstats["placed"], a.gstats["aligned_bases"], a.gstats["mismatches"], a.gstats["low_qual"], a.gstats["n_dropped"]) == \
               (b.stats["placed"], b.stats["bases"], b.stats["mismatches"], b.stats["low_qual"], b.stats["n_dropped"])
        ca, cb = pgc.GappedCalls(a), ck.Calls(b)
        for i, read, qual, p, g, j, inv in pgc._records(ca, h["b1"], h["b2"], h["gaps"]):
            if g == 0:
                ca.place_gapped(read, qual, p, g, j, inv)
                cb.place(read, qual, p, inv)
        assert np.array_equal(ca.cnt, cb.cnt) and np.array_equal(ca.qsum, cb.qsum)
        assert (ca.gstats["site_bases"], ca.gstats["site_low_qual"]) == (cb.stats["site_bases"], cb.stats["low_qual"])
    assert seen >= 40


def test_the_indel_calls_do_not_move(ora):
    """the indel checker fed depth - gdepth of a pileup with the gapped adds gives what it gives today on the pileup without them"""
    h = iw.hand_cases()
    cases = [(h["sym"], h["frag_start"], h["b1"], h["b2"], h["pairs"], h["gaps"], (h["pb1"], h["pb2"]))]
    sym, frag_start, b1, b2, pairs, rec = _planted(ora)
    cases.append((sym, frag_start, b1, b2, pairs, rec, (b1, b2)))
    for sym, frag_start, b1, b2, pairs, gaps, pb in cases:
        plain = pk.Pileup(sym, 0, 20)
        plain.add_pairs(*pb, pairs)
        today = ic.Indels(plain, frag_start)
        today.add(b1, b2, gaps)
        pu = pgc.GappedPileup(sym, 0, 20)
        pu.add_pairs(*pb, pairs)
        pu.add_gapped(b1, b2, gaps)
        assert np.array_equal(pu.depth - pu.gdepth, plain.depth) and not np.array_equal(pu.depth, plain.depth)
        then = ic.Indels(pu.ungapped_view(), frag_start)
        then.add(b1, b2, gaps)
        ic.assert_lists_equal(then.events(), today.events(), "events")
        ic.assert_lists_equal(then.calls(), today.calls(), "calls")
        assert then.finish_stats() == today.finish_stats() and today.events().shape[0] > 20
        # and fed the total depth they would move
        moved = ic.Indels(pu, frag_start)
        moved.add(b1, b2, gaps)
        assert not np.array_equal(moved.events()["ref_n"], today.events()["ref_n"])


def test_the_depth_does_not_dip_at_a_planted_deletion(ora):
    """what the stage is for: beside a planted homozygous deletion the depth comes back"""
    sym, frag_start, b1, b2, pairs, rec = _planted(ora)
    pu = pgc.GappedPileup(sym, 0, 20)
    pu.add_pairs(b1, b2, pairs)
    pu.add_gapped(b1, b2, rec)
    plain = pu.depth - pu.gdepth
    w = iw.planted()
    seen = 0
    for p in w.plants:
        if p["cls"] != "hom_del" or p["g"] < 2:
            continue
        x, g = p["x"], p["g"]
        flank = np.r_[x - 30:x - 5]
        assert pu.depth[flank].mean() > plain[flank].mean() + 3, (p, pu.depth[flank].mean(), plain[flank].mean())
        seen += 1
    assert seen >= 3


def test_exports_header_block_and_mirror():
    from real_amd import lib as rlib
    from real_amd.matcher import PairMatcher
    header = open(os.path.join(ROOT, "include", "real_hip.h")).read()
    assert "#define REAL_HIP_ABI_VERSION 2" in header
    assert "gapped placements in the pileup and the calls" in header and "holds only ungapped placements" not in header
    assert "u = depth - gdepth" in header and "bases + real_hip_pileup_gapped_stats::aligned_bases" in header
    hs = header_structs()
    assert hs["real_hip_pileup_gapped_stats"][:2] == ["struct_size", "reserved"]
    assert hs["real_hip_pileup_gapped_stats"][2:] == list(rlib.PILEUP_GAPPED_STATS_FIELDS)
    assert tuple(rlib.PILEUP_GAPPED_STATS_FIELDS[:-2]) == pgc.COUNTERS + pgc.CALL_COUNTERS
    assert C.sizeof(rlib.RealHipPileupGappedStats) == 8 + 15 * 8
    assert C.sizeof(rlib.RealHipPileupStats) == 8 + 13 * 8 and C.sizeof(rlib.RealHipGapPlace) == 16     # no struct grew
    L = rlib.load()
    for name in ("real_hip_pileup_add_gapped", "real_hip_call_add_gapped", "real_hip_pileup_depth_gapped", "real_hip_pileup_gapped_stats_get"):
        assert name in rlib.ABI_SYMBOLS and hasattr(L, name)
    assert L.real_hip_pileup_add_gapped(None, None, None, None) == rlib.REAL_HIP_E_INVALID
    assert L.real_hip_call_add_gapped(None, None, None, None) == rlib.REAL_HIP_E_INVALID
    assert L.real_hip_pileup_depth_gapped(None, 0, 0, None, 0) == rlib.REAL_HIP_E_INVALID
    assert L.real_hip_pileup_gapped_stats_get(None, None, 0) == rlib.REAL_HIP_E_INVALID
    for name in ("pileup_begin", "indel_add", "pileup_add_gapped", "call_add_gapped", "pileup_depth_gapped", "pileup_gapped_stats"):
        assert callable(getattr(PairMatcher, name))
    mk = open(os.path.join(ROOT, "real_amd", "csrc", "Makefile")).read()
    assert "pileup_gapped.o" in mk and "pileup_gapped_stage.h" in mk
    # the stage's state lives beside the ctx: the hashed header does not know it
    assert "gdiff" not in open(os.path.join(ROOT, "real_amd", "csrc", "real_hip_internal.h")).read()


def test_realoptions_pileup_gapped_flag_and_loud_refusals(tmp_path):
    """-pileup_gapped through the C++ parser (host_selftest pileup_gapped_options): what it needs, loudly, before any file is read"""
    import subprocess
    selftest = os.path.join(ROOT, "real_amd", "host", "host_selftest")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "real_amd", "host"), "host_selftest"], stdout=subprocess.DEVNULL)
    fa = tmp_path / "m2.fa"
    fa.write_text(">r\nACGT\n")
    base = ["-t", "g.fa", "-p", str(fa), "-o", "out", "-e", "3"]

    def run(args):
        return subprocess.run([selftest, "pileup_gapped_options"] + base + args, capture_output=True, text=True)
    for out in (["-pileup", "s.tsv"], ["-pileup_depth", "d.tsv"], ["-vcf", "x.vcf"]):
        r = run(["-p2", str(fa)] + out + ["-pileup_gapped", "1"])
        assert r.returncode == 0 and r.stdout.split() == ["1", "8", "8"], r.stderr
    assert run(["-p2", str(fa), "-pileup", "s.tsv"]).stdout.split()[0] == "0"
    assert run(["-p2", str(fa), "-pileup", "s.tsv", "-pileup_gapped", "0"]).stdout.split()[0] == "0"
    assert run(["-p2", str(fa), "-pileup", "s.tsv", "-pileup_gapped", "1", "-gap_max", "5", "-gap_flank", "9"]).stdout.split() == ["1", "5", "9"]
    for bad, word in ((["-pileup", "s.tsv", "-pileup_gapped", "1"], "single-end drivers are not there yet"),
                      (["-p2", str(fa), "-pileup_gapped", "1"], "needs one of -pileup / -pileup_depth / -vcf"),
                      (["-p2", str(fa), "-pileup", "s.tsv", "-pileup_gapped", "1", "-pairs_all", "1"], "-pairs_all"),
                      (["-p2", str(fa), "-pileup", "s.tsv", "-pileup_gapped", "1", "-gap_max", "17"], "-gap_max"),
                      (["-p2", str(fa), "-pileup", "s.tsv", "-pileup_gapped"], "missing")):
        r = run(bad)
        assert r.returncode == 1 and word in r.stderr, (bad, r.stderr)
    help_text = subprocess.run([selftest, "options", "-h"], capture_output=True, text=True).stderr
    assert "-pileup_gapped" in help_text and "do NOT apply to gapped placements" in help_text
    assert "-pileup_gapped" in open(os.path.join(ROOT, "README.md")).read()
