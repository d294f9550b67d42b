"""CPU checks that belong to the GPU instance matrix (tests/test_gpu_instances.py): the matrix covers every compiled
lane-matcher instance, and the oracle takes reads without qualities."""
import os
import re

import numpy as np

import test_gpu_instances as inst
from real_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_matrix_covers_every_compiled_instance():
    """W = 1..REAL_HIP_MAX_PATL / 32 x the lane matcher's table kinds x scores x mode, minus the declared exclusions: a
    width added to the Makefile, or a table kind added to the kernel, has to come with its cells."""
    max_patl = int(re.search(r"#define\s+REAL_HIP_MAX_PATL\s+(\d+)u?", _read("include", "real_hip.h")).group(1))
    max_w = max_patl // 32
    assert inst.MAX_W == max_w
    widths = re.search(r"^WIDTHS\s*:=\s*(.*)$", _read("real_amd", "csrc", "Makefile"), re.M).group(1).split()
    assert sorted(int(x) for x in widths) == list(range(1, max_w + 1)), "the Makefile builds widths the matrix does not know"
    enum = re.search(r"enum\s*:\s*int\s*\{([^}]*TK_STARTS[^}]*)\}", _read("real_amd", "csrc", "match_kernel.hip")).group(1)
    kinds = {e.split("=")[0].strip() for e in enum.split(",") if e.strip()}
    assert kinds == {g.tk for g in inst.GEOMETRIES.values()}, "a table kind of the kernel has no geometry"
    want = {(w, tk, s, mode) for w in range(1, max_w + 1) for tk in kinds for s in (0, 1) for mode in ("unique", "all")}
    have = {(c.w, inst.GEOMETRIES[c.geom].tk, c.scores, c.mode) for c in inst.CELLS}
    missing = want - have
    # what is missing is what the exclusions leave out, and nothing else
    declared = {(w, inst.GEOMETRIES[g].tk) for (w, g) in inst.EXCLUDED}
    assert {(w, tk) for (w, tk, _, _) in missing} <= declared, sorted(missing)
    assert missing == {(w, tk, s, md) for (w, tk) in declared for s in (0, 1) for md in ("unique", "all")} - have
    assert all(inst.GEOMETRIES[g].seedl > 32 * w for (w, g) in inst.EXCLUDED), "only cells whose read cannot hold a seed are left out"
    # one test per cell, named after it
    ids = [c.id for c in inst.CELLS]
    assert len(ids) == len(set(ids))
    # every geometry runs every width it can
    for name, g in inst.GEOMETRIES.items():
        ws = {c.w for c in inst.CELLS if c.geom == name}
        assert ws == {w for w in range(1, max_w + 1) if 32 * w >= g.seedl}, name


def test_oracle_without_qualities_scores_with_30(ora):
    """Reads without qualities (FASTA input) are scored with quality 30 (Pattern.hpp:42-45): the oracle with qual=None
    equals the oracle with an all-30 array, for matchUnique and matchAll."""
    g = synth.random_genome(60_000, seed=81, n_frag=2, n_runs=3, repeats=8)
    parts = [synth.sample_reads(g, 150, pl, 0.03, seed=82 + pl) for pl in (37, 100, 151)]
    b = synth.concat_batches(parts)
    og = ora.Genome(g.sym, g.frag_start)
    ix = ora.Index(og, 16)
    p = ora.make_params(seedl=16, seedkmax=2, totalkmax=5, scores=1)
    q30 = np.full(b.bases.shape[0], 30, dtype=np.uint8)
    ni, ns, nc = ora.match_unique(og, ix, p, b.bases, None, b.offsets)
    qi, qs, qc = ora.match_unique(og, ix, p, b.bases, q30, b.offsets)
    assert np.array_equal(ni, qi) and np.array_equal(ns.view(np.uint32), qs.view(np.uint32)) and nc == qc
    st = ora.unpack_record(ni)[0]
    assert ((st == 1) | (st == 2)).sum() > 200
    # the qualities do reach the score: the batch's own ones give other scores
    _, bs, _ = ora.match_unique(og, ix, p, b.bases, b.qual, b.offsets)
    assert not np.array_equal(bs.view(np.uint32), ns.view(np.uint32))
    nh, no, _ = ora.match_all(og, ix, p, b.bases, None, b.offsets)
    qh, qo, _ = ora.match_all(og, ix, p, b.bases, q30, b.offsets)
    assert np.array_equal(no, qo) and nh.shape[0] > 300
    assert nh.tobytes() == qh.tobytes()
