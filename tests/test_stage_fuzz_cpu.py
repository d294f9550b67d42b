"""The randomised stage chains without a device (tests/stage_fuzz.py): the generator is deterministic, the committed seeds of
test_gpu_stage_fuzz.py cover the drawn domain, every committed configuration gives every stage work (checked with the checkers
alone), the checkers' second formulations agree on the smallest configurations, the runner's comparison path names the stage of a
perturbed record, and the default workloads of the three generators that gained arguments are byte for byte what they were.

How the seeds were chosen: seeds 0 .. 799 of the paired kind and 0 .. 659 of the single kind were drawn; those that miss a floor
were dropped -- mostly because no gap record turned out NonUnique (class R shows its outcome in about half of the draws, and beside
a paired target only in an insert window wide enough for its second copy) or because fewer than ten records were gapped at a
tight max_cost -- and from the rest sixteen per kind were taken greedily until every value of the domain occurred.  SEEDS_DROPPED
names the seeds below the largest committed one that missed a floor.

Floors and short reads: a read shorter than 2 * min_flank + max_gap + 1 makes the gap stage skip it.  Such a configuration is
legitimate; the floors that count gap records (placed / unique / gapped, deletion, insertion, NonUnique, NoMatch, indel event) are
then replaced by skipped > 0, the others (duplicate, pileup site, mismatch list) stay."""
import copy

import numpy as np
import pytest

import dup_gapped_checker as dgk
import gap_anchor_checker as gac
import gap_anchor_workloads as aw
import gap_checker as gc
import gap_workloads as gw
import gapped_list_checker as glc
import pairs_checker as pc
import pileup_gapped_checker as pgc
import single_gapped_workloads as sgw
import singles_checker as sc
import stage_fuzz as sf
import test_gpu_stage_fuzz as committed

CONFIGS = [("paired", s) for s in committed.PAIRED_SEEDS] + [("single", s) for s in committed.SINGLE_SEEDS]
SEEDS_DROPPED = {
    "paired": (
        0, 2, 3, 4, 5, 7, 11, 12, 13, 15, 20, 21, 23, 25, 26, 28, 29, 30, 31, 32, 34, 37, 42, 43, 44, 49, 54, 56, 57,
        58, 60, 61, 62, 63, 65, 66, 69, 72, 75, 76, 77, 78, 79, 80, 82, 83, 84, 87, 90, 93, 97, 98, 101, 104, 105,
        107, 108, 109, 113, 115, 118, 119, 124, 125, 129, 130, 131, 133, 137, 139, 140, 142, 144, 145, 146, 147, 150,
        151, 152, 160, 163, 165, 168, 172, 175, 178, 179, 180, 181, 184, 185, 187, 188, 190, 191, 192, 193, 194, 196,
        197, 199, 203, 204, 207, 208, 210, 211, 213, 216, 217, 219, 222, 223, 224, 225, 227, 229, 230, 231, 233, 235,
        236, 238, 240, 241, 242, 244, 245, 248, 251, 254, 255, 258, 260, 261, 262, 263, 264, 265, 266, 267, 268, 269,
        270, 271, 272, 278, 279, 283, 284, 285, 287, 288, 289, 290, 292, 294, 297, 302, 304, 307, 309, 310, 312, 313,
        314, 315, 316, 317, 320, 323, 324, 326, 327, 328, 329, 332, 339, 342, 346, 348, 349, 351, 353, 354, 356, 357,
        360, 361, 362, 364, 365, 366, 368, 369, 370, 372, 376, 377, 378, 379, 380, 383, 384, 385, 386, 389, 393, 394,
        395, 396, 397, 399, 400, 401, 402, 404, 408, 411, 412, 414, 415, 417, 421, 423, 425, 427, 428, 429, 430, 431,
        433, 434, 437, 439, 442, 443, 444, 445, 449, 451, 452, 453, 460, 463, 464, 465, 467, 469, 470, 471, 474, 477,
        481, 482, 484, 488, 489, 490, 493, 494, 496, 497, 499, 500, 501, 502, 503, 504, 506, 509, 511, 513, 515, 516,
        517, 518, 519, 520, 521, 523, 524, 525, 528, 530, 532, 533, 536, 539, 540, 541, 544, 548, 550, 553, 554, 557,
        558, 559, 560, 561, 562, 563, 564, 569, 570, 572, 574, 578, 579, 580, 581, 583, 585, 587, 591, 593, 594, 595,
        597, 599, 600, 602, 605, 608, 609, 613, 616, 618, 620, 622, 623, 624, 625, 626, 627, 632, 635, 637, 638, 639,
        642, 643, 644, 645, 646, 647, 648, 650, 651, 652, 653, 655, 656, 657, 660, 661, 662, 665, 667, 669, 671, 673,
        675, 677, 678, 680, 683, 685, 686, 688, 690, 692, 693, 697, 701, 702, 704, 705, 706, 711, 712, 713, 716, 724,
        725, 726, 728, 729, 733, 734, 736, 737, 740, 741, 742, 744, 747, 748, 750, 751, 753, 755, 756, 757, 759, 763,
        764, 765, 766, 767, 769, 772, 776, 777, 778, 782, 785, 786, 788, 789, 792, 794, 795),
    "single": (
        5, 7, 10, 12, 16, 19, 20, 21, 22, 23, 26, 28, 30, 31, 34, 35, 38, 39, 40, 42, 43, 44, 45, 49, 52, 53, 55, 56,
        62, 63, 68, 69, 72, 79, 86, 87, 93, 97, 99, 101, 104, 107, 110, 111, 114, 116, 119, 123, 125, 127, 128, 131,
        132, 134, 135, 136, 142, 148, 149, 150, 151, 162, 164, 166, 168, 169, 175, 188, 190, 191, 193, 195, 196, 198,
        199, 202, 203, 205, 206, 207, 215, 216, 220, 221, 222, 223, 224, 226, 228, 229, 231, 232, 236, 237, 239, 242,
        243, 251, 252, 253, 254, 255, 256, 257, 258, 261, 263, 264, 266, 269, 270, 273, 274, 276, 277, 278, 279, 281,
        283, 285, 291, 299, 301, 302, 303, 305, 307, 314, 315, 320, 323, 327, 329, 333, 335, 337, 339, 342, 343, 345,
        346, 348, 350, 353, 354, 355, 357, 358, 372, 373, 377, 378, 396, 397, 402, 407, 408, 417, 419, 420, 422, 426,
        433, 442, 444, 453, 458, 461, 462, 463, 468, 470, 471, 476, 477, 478, 482, 483, 484, 485, 486, 487, 488, 491,
        492, 494, 498, 505, 516, 522, 523, 524, 527, 529, 538, 546, 547, 548, 550, 551, 552, 557, 564, 565, 568, 572,
        575, 577, 579, 580, 581, 585, 588, 592, 593, 596, 598, 600, 602, 606, 607, 609, 616, 622, 625, 628, 630, 633,
        634, 636, 645, 646, 647, 648, 649, 651),
}

# sha256 of bases, qualities, offsets (of every batch) and the genome's symbols and fragment starts, computed on the commit before
# the generators took a seed length, mismatch bounds, an anchor-mate length and a quality generator
DEFAULTS = {"gap_workloads": "aa768ceef75b04fa77714d93a57a78f56d7cda83149a0d3561ac9ed6281df372",
            "gap_anchor_workloads": "a598b3db92bbbc084491ce29816de412e6e47a3bef5ca446d29d03696457100f",
            "single_gapped_workloads": "d33476d7fa7029a2c41903105b66d78a91cfb8f3e3cc7fe222cca62eb97a98d5"}


def test_the_default_workloads_are_byte_for_byte_what_they_were():
    w = gw.workload()
    assert sf.workload_digest(w["b1"].bases, w["b1"].qual, w["b1"].offsets, w["b2"].bases, w["b2"].qual, w["b2"].offsets, w["g"].sym,
                              w["g"].frag_start) == DEFAULTS["gap_workloads"]
    w = aw.workload()
    assert sf.workload_digest(w["b"].bases, w["b"].qual, w["b"].offsets, w["g"].sym, w["g"].frag_start) == DEFAULTS["gap_anchor_workloads"]
    w = sgw.workload()
    assert sf.workload_digest(w.b.bases, w.b.qual, w.b.offsets, w.g.sym, w.g.frag_start) == DEFAULTS["single_gapped_workloads"]
    # a part of a batch keeps its qualities
    b = gw.Batch([np.arange(5) % 4, np.arange(7) % 4], qual=lambda n: np.arange(n))
    assert b.part(1, 2).qual.tolist() == list(range(7)) and gw.Batch([np.zeros(3)]).part(0, 1).qual.tolist() == [35] * 3


def test_sixteen_seeds_of_each_kind_are_committed():
    assert len(committed.PAIRED_SEEDS) == len(set(committed.PAIRED_SEEDS)) == 16 and len(committed.SINGLE_SEEDS) == len(set(committed.SINGLE_SEEDS)) == 16
    assert not set(SEEDS_DROPPED["paired"]) & set(committed.PAIRED_SEEDS) and not set(SEEDS_DROPPED["single"]) & set(committed.SINGLE_SEEDS)


@pytest.mark.parametrize("kind,seed", CONFIGS, ids=lambda v: str(v))
def test_draw_and_workload_are_functions_of_kind_and_seed(kind, seed):
    cfg = sf.draw(kind, seed)
    assert cfg == sf.draw(kind, seed) and repr(cfg) == repr(sf.draw(kind, seed))
    first = sf.digest_of(cfg)
    sf._WORK.pop((kind, seed))
    assert sf.digest_of(cfg) == first
    assert cfg != sf.draw(kind, seed + 1) and cfg != sf.draw("single" if kind == "paired" else "paired", seed)


def test_every_drawn_value_lies_inside_what_the_library_accepts():
    for kind, seed in CONFIGS:
        c = sf.draw(kind, seed)
        assert c.seedl in sf.SEEDLS and c.seedl % 4 == 0 and not (c.seedl == 32 and c.table_kind == 3)
        assert 0 <= c.seedkmax <= min(2, c.totalkmax) and 1 <= c.totalkmax <= 6 and c.filter_level in sf.FILTER_LEVELS
        assert 1 <= c.max_gap <= gc.GAP_MAX and 1 <= c.min_flank <= 12 and c.margin in sf.MARGINS
        assert c.max_cost is None or 6 + c.max_gap <= c.max_cost <= 4 * c.totalkmax + 6 + c.max_gap
        assert 100_000 <= c.size <= 200_000 and 2 <= c.n_frag <= 8 and 0 <= c.n_runs <= 6 and 65 <= c.n <= 150
        assert len(set(c.fileids)) == len(c.fileids) in (1, 2) and set(c.fileids) <= set(sf.FILE_IDS)
        assert 2 <= c.hist_bins <= 16384 and c.patl in sf.TARGET_LENGTHS and c.patl <= gc.MAX_PATL
        if kind == "paired":
            assert c.patl + c.anchor_l <= c.frag_l == c.min_ins <= c.max_ins <= sf.MATE_SEARCH_MAX_INSERT and c.anchor_l in sf.ANCHOR_MATE_LENGTHS
        else:
            assert max(c.seedl, 32) <= c.anchor_len <= gc.MAX_PATL and 1 <= c.max_anchors <= gac.ANCHORS_MAX and 1 <= c.n_blocks <= 3
        w = sf.workload(c)
        assert 0 <= w.cut <= w.n and (c.cut != "inside" or 0 < w.cut < w.n)


def test_the_committed_seeds_cover_the_domain():
    cfgs = [sf.draw(k, s) for k, s in CONFIGS]
    paired, single = [c for c in cfgs if c.kind == "paired"], [c for c in cfgs if c.kind == "single"]

    def seen(name, among=cfgs):
        return {getattr(c, name) for c in among}
    listed = dict(seedl=sf.SEEDLS, layout=sf.LAYOUTS, seedkmax=(0, 1, 2), totalkmax=range(1, 7), scores=(0, 1), filter_level=sf.FILTER_LEVELS,
                  margin=sf.MARGINS, pileup_minq=sf.PILEUP_MINQ, min_call_qual=sf.MIN_CALL_QUAL, min_depth=sf.MIN_DEPTH, min_alt=sf.MIN_ALT,
                  dedup_minq=sf.DEDUP_MINQ, hist_bins=sf.HIST_BINS, presentation=sf.PRESENTATIONS, garbage_out=(0, 1), cut=sf.CUTS,
                  gapped_first=(0, 1), second_half_first=(0, 1), dedup=(0, 1), patl=sf.TARGET_LENGTHS,
                  max_gap=range(1, 17), min_flank=range(1, 13), n_frag=range(2, 9), n_runs=range(0, 7))
    for name, values in listed.items():
        assert seen(name) >= set(values), (name, sorted(set(values) - seen(name)))
    for among in (paired, single):                                        # what matters to each chain on its own
        for name in ("scores", "presentation", "cut", "layout", "patl"):
            assert seen(name, among) >= set(listed[name]), (among[0].kind, name, sorted(set(listed[name]) - seen(name, among)))
        assert {len(c.fileids) for c in among} == {1, 2}
    assert {f for c in cfgs for f in c.fileids} == set(sf.FILE_IDS)
    assert {c.qual_const is None for c in cfgs} == {True, False} and {c.max_cost is None for c in cfgs} == {True, False}
    assert seen("anchor_l", paired) == set(sf.ANCHOR_MATE_LENGTHS) and {c.window for c in paired} >= set(sf.WINDOWS)
    assert seen("mate_search", paired) == {0, 1} and {c.search_anchors for c in paired if c.mate_search} == set(sf.SEARCH_ANCHORS)
    assert seen("max_anchors", single) == set(sf.SINGLE_ANCHORS) and seen("n_blocks", single) == {1, 2, 3}


_FLOORS = {}
BRUTE = 10              # the reads the brute-force formulation is held against: the first plant of every class


def _floors(ora, kind, seed):
    if (kind, seed) not in _FLOORS:
        cfg = sf.draw(kind, seed)
        _FLOORS[(kind, seed)] = sf.floors(cfg, sf.expected(cfg, ora))
    return _FLOORS[(kind, seed)]


@pytest.mark.parametrize("kind,seed", CONFIGS, ids=lambda v: str(v))
def test_every_configuration_gives_every_stage_work(ora, kind, seed):
    f = _floors(ora, kind, seed)
    print(f)
    sf.assert_floors(sf.draw(kind, seed), f)


def test_the_list_as_a_whole_reaches_the_calls_the_search_and_low_mapq(ora):
    total = {}
    for kind, seed in CONFIGS:
        for k, v in _floors(ora, kind, seed).items():
            total[k] = total.get(k, 0) + v
    assert total["snp_calls"] >= 1 and total["indel_calls"] >= 1 and total["searched_changed"] >= 1 and total["mapq_below_60"] >= 1, total
    for kind in ("paired", "single"):                                     # and each chain on its own
        own = [_floors(ora, k, s) for k, s in CONFIGS if k == kind]
        assert sum(f["snp_calls"] for f in own) >= 1 and sum(f["indel_calls"] for f in own) >= 1
    # (a MAPQ below 60 comes from the single chain alone: the paired workloads plant no repeat that both mates hit ungapped, so
    # every placed fragment of theirs has one candidate -- none of 163 drawn paired configurations that met the floors had another)
    assert sum(_floors(ora, k, s)["mapq_below_60"] for k, s in CONFIGS if k == "single") >= 1


def _volume(cfg):
    """the triples (start, gap, split) times the read length: what the brute-force formulation walks per searched read"""
    starts = (cfg.window if cfg.kind == "paired" else 1) + 2 * cfg.max_gap
    return starts * (2 * cfg.max_gap + 1) * max(1, cfg.patl - 2 * cfg.min_flank) * cfg.patl if cfg.searched else 1 << 60


def _smallest(kind):
    """the two configurations of a kind with the least work for the brute-force formulation"""
    return sorted((s for k, s in CONFIGS if k == kind), key=lambda s: (_volume(sf.draw(kind, s)), s))[:2]


def test_the_second_formulations_agree_on_the_smallest_configurations(ora):
    for seed in _smallest("paired"):
        cfg = sf.draw("paired", seed)
        w, exp = sf.workload(cfg), sf.expected(cfg, ora)
        b1, b2 = w.b1, w.b2
        l1, l2 = np.diff(b1.offsets.astype(np.int64)), np.diff(b2.offsets.astype(np.int64))
        fm = ora.filter_mult(cfg.filter_level, cfg.totalkmax)
        files = exp["_files"]
        pc.assert_records_equal(pc.naive_pairs(files, l1, l2, cfg.min_ins, cfg.max_ins, bool(cfg.scores), fm), exp["_plain_pairs"], "naive_pairs")
        first = exp["match_pairs_singles"]
        sc.assert_singles_equal(sc.sorted_singles([(f[0], f[1], f[2]) for f in files], l1, bool(cfg.scores), fm), first["singles1"], "sorted_singles")
        sc.assert_singles_equal(sc.sorted_singles([(f[0], f[3], f[4]) for f in files], l2, bool(cfg.scores), fm), first["singles2"], "sorted_singles")
        gaps, k = None, BRUTE                                             # (the brute force walks every triple: the first plants, one of each class)
        for fid, g in w.files[::-1]:
            gaps, _ = gc.check_gap(gc.Text(g.sym, g.frag_start, fid), b1.part(0, k), b2.part(0, k), first["pairs"][:k], first["singles1"][:k],
                                   first["singles2"][:k], cfg.min_ins, cfg.max_ins, cfg.prm, out=gaps, candidates=gc.brute_candidates)
        gc.assert_records_equal(gaps, exp["gap_rescue"]["gaps"][:k], "brute_candidates")
        _gapped_consumers_again(cfg, w, exp, (b1, b2), exp["gap_rescue"]["gaps"])
    for seed in _smallest("single"):
        cfg = sf.draw("single", seed)
        w, exp = sf.workload(cfg), sf.expected(cfg, ora)
        info = exp["match_unique"]["info"]
        some, k = None, BRUTE
        for fid, g, _, _, hs, os_ in exp["_lists"]:
            some, _ = gac.check_anchor(gc.Text(g.sym, g.frag_start, fid), w.b.part(0, k), info[:k], hs, os_[:2 * k + 1], cfg.prm,
                                       gac.AnchorParams(cfg.anchor_len, cfg.max_anchors), out=some, candidates=gc.brute_candidates, union=gac.best_second_fold)
        gaps = exp["match_gapped"]["gaps"]
        gc.assert_records_equal(some, gaps[:k], "brute_candidates, best_second_fold")
        dup, st = dgk.mark_sorted(info, gaps, exp["duplicates"]["sums"])
        assert np.array_equal(dup, exp["duplicates"]["dup_gapped"]) and st == exp["duplicates"]["stats_gapped"], "mark_sorted"
        placed = dgk.masked_gaps(gaps, exp["duplicates"]["dup_gapped"]) if cfg.dedup else gaps
        _gapped_consumers_again(cfg, w, exp, (w.b, w.b), gaps, placed)


def _gapped_consumers_again(cfg, w, exp, mates, gaps, placed=None):
    """list_by_diagonals and aligned_by_diagonals against the formulations expected() used"""
    lists, off, st = glc.gapped_lists(w.main.sym, w.main_fid, *mates, gaps, one_list=glc.list_by_diagonals)
    want = exp["mismatches_gapped"]
    assert lists.tobytes() == want["lists"].tobytes() and np.array_equal(off, want["offsets"]) and st == want["stats"], "list_by_diagonals"
    pu = pgc.GappedPileup(w.main.sym, w.main_fid, cfg.pileup_minq, aligned=pgc.aligned_by_diagonals)
    pu.add_gapped(*mates, gaps if placed is None else placed)
    first = pgc.GappedPileup(w.main.sym, w.main_fid, cfg.pileup_minq)
    first.add_gapped(*mates, gaps if placed is None else placed)
    assert np.array_equal(pu.depth, first.depth) and np.array_equal(pu.gdepth, exp["pileup"]["gdepth"]) and pu.gapped_stats() == first.gapped_stats(), \
        "aligned_by_diagonals"


@pytest.mark.parametrize("kind,stage", [("paired", "gap_rescue"), ("single", "match_gapped")])
def test_a_perturbed_record_of_a_late_stage_is_named(ora, kind, stage):
    """the runner's comparison path: split + 1 in one Unique gap record, one depth, one counter -- each raises with the stage's name
    and the configuration; the untouched output passes"""
    seed = _smallest(kind)[0]
    cfg = sf.draw(kind, seed)
    exp = sf.expected(cfg, ora)
    sf.check_stage(cfg, stage, copy.deepcopy(exp[stage]), exp[stage])
    got = copy.deepcopy(exp[stage])
    unique = np.nonzero((gc.state_of(got["gaps"]["tag"]) == gc.UNIQUE) & (got["gaps"]["gap"] != 0))[0]
    got["gaps"]["split"][unique[-1]] += 1
    with pytest.raises(sf.StageDiff) as e:
        sf.check_stage(cfg, stage, got, exp[stage])
    assert e.value.stage == stage and ("stage %s differs" % stage) in str(e.value) and repr(cfg) in str(e.value) and "seed=%d" % seed in str(e.value)
    assert "split" in str(e.value)
    for late, key, change in (("pileup", "depth", lambda a: a.__setitem__(int(np.nonzero(a)[0][0]), a[np.nonzero(a)[0][0]] + 1)),
                              ("indels", "stats", lambda d: d.__setitem__("events", d["events"] + 1)),
                              ("calls", "evidence", lambda a: a["qsum"].__setitem__((0, 0), a["qsum"][0, 0] + 1))):
        got = copy.deepcopy(exp[late])
        change(got[key])
        with pytest.raises(sf.StageDiff) as e:
            sf.check_stage(cfg, late, got, exp[late])
        assert e.value.stage == late and repr(cfg) in str(e.value) and key in str(e.value)
