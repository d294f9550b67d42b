"""Single-end gapped reads in SAM, pileup and VCF, and duplicates across gapped and ungapped reads, without a GPU:
the two formulations of the joint marking against each other and against dup_checker; END5 by hand; the floors of the workload,
so that no GPU test passes vacuously; RealOptions through host_selftest; the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dup_checker as dk
import dup_gapped_checker as dgk
import gap_checker as gc
import indel_workloads as iw
import single_gapped_checker as sgc
import single_gapped_workloads as sw
from real_amd import lib as rlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the marking ---------------------------------------------------------------------------------------------------------------
def _both(info, gaps, sums):
    a, b = dgk.mark_groups(info, gaps, sums), dgk.mark_sorted(info, gaps, sums)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    return a


@pytest.mark.parametrize("n", sw.HAND_N)
def test_the_two_formulations_agree_on_hand_arrays(n):
    info, gaps, sums = sw.hand(n)
    dup, st, groups = _both(info, gaps, sums)
    assert st["placed"] - st["groups"] == int(dup.sum()) and (n < 255 or st["duplicates"] > 50)


def test_the_two_formulations_agree_on_the_edges_and_the_workload(ora):
    info, gaps, sums, want = sw.hand_edges()
    assert _both(info, gaps, sums)[0].tolist() == want.tolist()
    info, gaps, sums, dup, st, _ = sw.expected(ora)
    got = dgk.mark_sorted(info, gaps, sums)
    assert np.array_equal(got[0], dup) and got[1] == st


def test_without_a_unique_gap_record_it_is_the_single_end_marking():
    info, gaps, sums = sw.hand(4099)
    nonunique = gaps.copy()
    nonunique["tag"] = (nonunique["tag"] & ~np.uint8(3 << 5)) | np.uint8(gc.NONUNIQUE << 5)
    for g in (gc.empty_records(4099), nonunique):
        dup, st, _ = _both(info, g, sums)
        want = dk.mark_single(info, sums)
        assert np.array_equal(dup, want[0]) and st == want[1] and st["duplicates"] > 100
    assert not np.array_equal(_both(info, gaps, sums)[0], dk.mark_single(info, sums)[0])


@pytest.mark.parametrize("inv", [0, 1])
@pytest.mark.parametrize("g", [-3, 4, 0])
def test_end5_by_hand(inv, g):
    """forward: pos; reverse: pos + len + gap - 1 -- the last text position of the span"""
    gaps = gc.empty_records(1)
    gaps["pos"], gaps["gap"], gaps["tag"], gaps["fileid"] = 1000, g, dgk.gap_tag(gc.UNIQUE, inv), 5
    sums = np.array([(100, 3000)], dtype=dk.SUM_DTYPE)
    want = {(0, -3): 1000, (0, 4): 1000, (0, 0): 1000, (1, -3): 1096, (1, 4): 1103, (1, 0): 1099}[(inv, g)]
    assert dgk.keys(np.zeros(1, dtype=np.uint64), gaps, sums) == [(5, inv, want)]
    # an ungapped read with that 5' end has that key: state 2 at pos = END5 - len + 1, state 1 at END5
    info = np.array([sw.info_word(2, want - 60 + 1, 5) if inv else sw.info_word(1, want, 5)], dtype=np.uint64)
    assert dgk.keys(info, gc.empty_records(1), np.array([(60, 1)], dtype=dk.SUM_DTYPE)) == [(5, inv, want)]


def test_the_info_word_wins_and_nonunique_places_nothing():
    gaps = gc.empty_records(3)
    gaps["pos"], gaps["tag"] = 500, dgk.gap_tag(gc.UNIQUE, 0)
    gaps["tag"][2] = dgk.gap_tag(gc.NONUNIQUE, 0)
    info = np.array([sw.info_word(1, 900), 0, 0], dtype=np.uint64)
    sums = np.array([(50, 10)] * 3, dtype=dk.SUM_DTYPE)
    assert dgk.keys(info, gaps, sums) == [(0, 0, 900), (0, 0, 500), None]
    assert dgk.placements(info, gaps, sums)[0].tolist() == [dgk.UNGAPPED, dgk.GAPPED, 0]
    assert dgk.gapped_line(info, gaps, sums) == "duplicates gapped: placements=2 duplicates=0"


# ---- the floors of the workload ------------------------------------------------------------------------------------------------
def test_the_workload_has_what_the_gpu_tests_need(ora):
    w = sw.workload()
    info, gaps, sums, dup, st, groups = sw.expected(ora)
    assert w.b.n_reads == 10317 and w.n_base == 8842
    state = gc.state_of(gaps["tag"])
    assert int(((state == gc.UNIQUE) & (gaps["gap"] != 0)).sum()) >= 400
    assert not ((state == gc.UNIQUE) & ((info >> np.uint64(61)) != 0)).any()           # (a gap record only where the matcher placed nothing)
    kinds = dgk.group_kinds(info, gaps, sums)
    alone = [k for k, (u, g) in kinds.items() if not u]
    mixed = [k for k, (u, g) in kinds.items() if u and g]
    assert len(alone) >= 50 and len(mixed) >= 50
    assert sum(1 for k in mixed if k[1] == 0) >= 20 and sum(1 for k in mixed if k[1] == 1) >= 20
    # the planted loci are called from the single reads, and the marks change what is counted
    pu, cl, ind = sgc.file_expected(w.g, 0, w.b, info, gaps)
    calls = ind.calls()
    called = {(int(c["pos"]), int(c["gap"]), int(c["seq"])) for c in calls}
    per_class = {}
    for p in w.plants:
        per_class[p["cls"]] = per_class.get(p["cls"], 0) + (iw.planted_key(w.planted, p) in called)
    assert set(per_class) == set(iw.P_CLASSES) and all(v >= 5 for v in per_class.values()), per_class
    pu2, cl2, ind2 = sgc.file_expected(w.g, 0, w.b, info, gaps, dup)
    marked = {(int(c["pos"]), int(c["gap"]), int(c["seq"])): (int(c["ref_n"]), int(c["alt_n"])) for c in ind2.calls()}
    assert any(k in marked and marked[k] != (int(c["ref_n"]), int(c["alt_n"])) for c in calls for k in [(int(c["pos"]), int(c["gap"]), int(c["seq"]))])
    assert pu2.gstats["placed"] < pu.gstats["placed"] and pu.gstats["deleted"] > 100 and pu.gstats["inserted"] > 100
    # the -sam text: a gapped line per Unique record, the marked ones with 1024
    text, ctrs = sgc.sam_single_gapped([w.g], w.b, info, gaps, dup)
    lines = [l.split("\t") for l in text.split("\n") if l and not l.startswith("@")]
    assert len(lines) == w.b.n_reads
    gapped = [f for f in lines if any(t.startswith("ZC:i:") for t in f[11:])]
    assert len(gapped) == int((state == gc.UNIQUE).sum()) and {int(f[1]) for f in gapped} == {0, 16, 1024, 1040}
    assert sum(1 for f in gapped if "D" in f[5]) >= 100 and sum(1 for f in gapped if "I" in f[5]) >= 100
    assert sgc.sam_gapped_line(ctrs).startswith("sam gapped: reads=%d " % len(gapped)) and sgc.sam_gapped_line(ctrs).endswith("disagree=0")


# ---- RealOptions ---------------------------------------------------------------------------------------------------------------
def test_realoptions_single_end_consumers(tmp_path):
    selftest = os.path.join(ROOT, "real_amd", "host", "host_selftest")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "real_amd", "host"), "host_selftest"], stdout=subprocess.DEVNULL)
    fa = tmp_path / "m2.fa"
    fa.write_text(">r\nACGT\n")
    base = ["-t", "g.fa", "-p", str(fa), "-o", "out", "-e", "3"]

    def run(args):
        return subprocess.run([selftest, "single_gapped_options"] + base + args, capture_output=True, text=True)
    gs = ["-gapped_single", "g.tsv"]
    for args, want in ((gs + ["-sam", "x.sam", "-sam_gapped", "1"], ["1", "0", "0", "0", "g.tsv"]),
                       (gs + ["-vcf", "x.vcf", "-vcf_indels", "1"], ["0", "1", "0", "0", "g.tsv"]),
                       (gs + ["-pileup", "s.tsv", "-pileup_gapped", "1"], ["0", "0", "1", "0", "g.tsv"]),
                       (gs + ["-pileup_depth", "d.tsv", "-pileup_gapped", "1", "-dedup", "1"], ["0", "0", "1", "1", "g.tsv"]),
                       (gs + ["-vcf", "x.vcf", "-pileup_gapped", "1", "-vcf_indels", "1", "-sam", "x.sam", "-sam_gapped", "1", "-dedup", "1"], ["1", "1", "1", "1", "g.tsv"]),
                       (gs, ["0", "0", "0", "0", "g.tsv"]), ([], ["0", "0", "0", "0", "."])):
        r = run(args)
        assert r.returncode == 0 and r.stdout.split() == want, (args, r.stdout, r.stderr)
    for bad, words in ((["-sam", "x.sam", "-sam_gapped", "1"], ["-sam_gapped", "-p2", "needs -gapped_single"]),
                       (["-vcf", "x.vcf", "-vcf_indels", "1"], ["-vcf_indels", "-p2", "needs -gapped_single"]),
                       (["-pileup", "s.tsv", "-pileup_gapped", "1"], ["-pileup_gapped", "needs -gapped_single", "single-end drivers are not there yet"]),
                       (gs + ["-sam_gapped", "1"], ["-sam_gapped", "needs -sam"]),
                       (gs + ["-vcf_indels", "1"], ["-vcf_indels", "needs -vcf"]),
                       (gs + ["-pileup_gapped", "1"], ["needs one of -pileup / -pileup_depth / -vcf"]),
                       # the -p2 rules are what they were
                       (["-p2", str(fa), "-sam", "x.sam", "-sam_gapped", "1"], ["-sam_gapped", "needs -gapped"]),
                       (["-p2", str(fa)] + gs + ["-vcf", "x.vcf", "-vcf_indels", "1"], ["-gapped_single places single reads"]),
                       (["-p2", str(fa), "-vcf_indels", "1"], ["needs -vcf"]),
                       (["-p2", str(fa), "-pileup_gapped", "1"], ["needs one of -pileup / -pileup_depth / -vcf"])):
        r = run(bad)
        assert r.returncode == 1 and all(w in r.stderr for w in words), (bad, r.stderr)
    for ok in (["-p2", str(fa), "-sam", "x.sam", "-gapped", "g.tsv", "-sam_gapped", "1"], ["-p2", str(fa), "-vcf", "x.vcf", "-vcf_indels", "1"],
               ["-p2", str(fa), "-pileup", "s.tsv", "-pileup_gapped", "1"]):
        assert run(ok).returncode == 0, ok
    help_text = subprocess.run([selftest, "options", "-h"], capture_output=True, text=True).stderr
    assert help_text.count("WITHOUT -p2 (it then needs") >= 3 and "-dedup 1 DOES apply" in help_text and "do NOT apply to gapped placements" in help_text
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "without `-p2`" in readme and "-gapped_single" in readme and "duplicates gapped:" in readme


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_joint_marking():
    name = "real_hip_mark_duplicates_gapped"
    hdr = open(os.path.join(ROOT, "include", "real_hip.h")).read()
    assert ("int %s(real_hip_ctx *ctx, const uint64_t *info, const struct real_hip_gap_place *gaps," % name) in hdr
    assert "#define REAL_HIP_ABI_VERSION 2" in hdr.replace("  ", " ")
    assert name in rlib.ABI_SYMBOLS
    L = rlib.load()
    assert L.real_hip_abi_version() == 2 and hasattr(L, name)
    assert L.real_hip_mark_duplicates_gapped(None, None, None, None, 1, 0, None) == rlib.REAL_HIP_E_INVALID       # a NULL ctx
    assert C.sizeof(rlib.RealHipDupStats) == 56 and rlib.GAP_PLACE_DTYPE.itemsize == 16 and rlib.READ_SUM_DTYPE.itemsize == 8
    from real_amd.matcher import HipMatcher
    assert callable(HipMatcher.mark_duplicates_gapped)
    # the launcher is declared in the stage's header, its record is a member of the ctx: the header bench.py hashes knows neither
    csrc = os.path.join(ROOT, "real_amd", "csrc")
    assert "mark_duplicates_gapped" not in open(os.path.join(csrc, "real_hip_internal.h")).read()
    assert "rh_launch_mark_duplicates_gapped" in open(os.path.join(csrc, "dup_gapped_stage.h")).read()
    assert "RhDupGappedStage dup_gapped;" in open(os.path.join(csrc, "real_hip_ctx.h")).read()
    assert "dup_gapped_stage.h" in open(os.path.join(csrc, "Makefile")).read()
