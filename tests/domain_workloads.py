"""The edges of the batch domain as one seeded workload -- TEST INFRASTRUCTURE ONLY: reads of every length at which a kernel
changes form (LENS), quality bytes 0..127 with a 0..63 twin, reads without bases.  test_batch_domain_cpu.py shows with the
oracle alone that the workload holds what it claims; the GPU tests compare the library with the oracle on it.

The genome (200 kbp, two fragments, two runs of N) holds one exact second copy of a 17000-base stretch and one near copy of
another, which differs from its source at two bases per 2000.  Per length and strand a read lies on a fragment's first base,
ends on the text's last base, lies mid-text, on the exact copy's source and on the near copy's source; per length one read
holds an N, one has TOTALKMAX substitutions (offset 0, offset L - 1 and the base at which the wave kernel's 2048-base turn
ends -- or a middle base where the read is shorter) and one has one more."""
from __future__ import annotations

import types

import numpy as np

from real_amd import synth

LENS = (0, 31, 32, 320, 321, 2047, 2048, 2049, 4096, 16383, 16384)
UNIFORM = (2048, 2049, 16384)
SEEDKMAX, TOTALKMAX = 2, 3
N_GENOME, CUT = 200_000, 100_000
N_RUNS = ((90_000, 90_007), (170_000, 170_003))
COPY_LEN = 17_000
EXACT_SRC, EXACT_DST = 2_000, 120_000
NEAR_SRC, NEAR_DST = 20_000, 140_000
NEAR_EVERY, NEAR_FIRST = 1000, 500              # the near copy differs at offsets 500, 1500, ...: two per 2000 bases
P_MID, P_EXACT, P_NEAR, P_KMAX, P_OVER, P_N = 50_000, EXACT_SRC + 100, NEAR_SRC + 490, 50_500, 51_000, 51_500
FORCED_Q = (63, 64, 93, 127)
N_FILL, FILL_LEN = 300, 100
PAIR_LENS = ((2049, 100), (100, 16384), (0, 100), (100, 31))
PAIR_GAP = 100                                  # bases between the mates of a fragment
KINDS = ("first", "end", "mid", "exact", "near")


def genome():
    rng = np.random.default_rng(2024)
    sym = rng.integers(0, 4, size=N_GENOME, dtype=np.uint8)
    sym[EXACT_DST:EXACT_DST + COPY_LEN] = sym[EXACT_SRC:EXACT_SRC + COPY_LEN]
    near = sym[NEAR_SRC:NEAR_SRC + COPY_LEN].copy()
    at = np.arange(NEAR_FIRST, COPY_LEN, NEAR_EVERY)
    near[at] = (near[at] + 1 + rng.integers(0, 3, size=at.shape[0])) & 3
    sym[NEAR_DST:NEAR_DST + COPY_LEN] = near
    for lo, hi in N_RUNS:
        sym[lo:hi] = 4
    return synth.Genome(sym=sym, frag_start=np.array([0, CUT, N_GENOME], dtype=np.uint64), frag_names=[" domain_0", " domain_1"])


def subst_offsets(L: int, k: int):
    """where a read of L bases gets k substitutions: its first and last base, the last base of the 2048-base turn (the base
    behind it where that is the read's last one; a middle base in a shorter read), then bases in the read's first third"""
    if L > 2049:
        third = 2048
    elif L == 2049:
        third = 2047
    else:
        third = L // 2 + 1
    out = [0, L - 1, third]
    j = L // 3
    while len(out) < k:
        if j not in out:
            out.append(j)
        j += 1
    return sorted(out[:k])


def _qualities(rng, L: int):
    q = rng.integers(0, 128, size=L, dtype=np.uint8)
    if L >= 16:
        for j, v in enumerate(FORCED_Q):
            q[1 + 4 * j] = v
            q[L - 2 - 4 * j] = v
    return q


def _batch(reads, ids=None):
    """reads: [(bases, qual)] -> ReadBatch"""
    lens = [r[0].shape[0] for r in reads]
    cat = lambda k: np.concatenate([r[k] for r in reads]).astype(np.uint8) if reads else np.zeros(0, np.uint8)
    return synth.ReadBatch(bases=cat(0), qual=cat(1), offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), ids=ids)


def twin(b):
    """the same reads with qualities q & 63"""
    return synth.ReadBatch(bases=b.bases, qual=(b.qual & 63).astype(np.uint8), offsets=b.offsets, ids=b.ids,
                           true_pos=b.true_pos, true_inv=b.true_inv)


def subset(b, idx):
    reads = [(b.bases[int(b.offsets[i]):int(b.offsets[i + 1])], b.qual[int(b.offsets[i]):int(b.offsets[i + 1])]) for i in idx]
    return _batch(reads, ids=None if b.ids is None else [b.ids[i] for i in idx])


def lens_of(b):
    return np.diff(b.offsets.astype(np.int64))


_W = None


def workload():
    """-> namespace: g; b (the ragged 0..127 batch) and b63 (its twin); meta[i] = (length, kind, strand, position) of read i
    (kind: one of KINDS, "n", "kmax", "over", "empty", "fill"); uniform[L] = the reads of length L as one batch of uniform
    length; empty (reads without bases only), edge_empty (first and last read empty); pairs = (mate batch 1, mate batch 2),
    pair_meta[i] = (start, outer distance, mate 1 is the forward mate)"""
    global _W
    if _W is not None:
        return _W
    g = genome()
    rng = np.random.default_rng(7)
    reads, meta = [], []

    def take(p, L, inv):
        r = g.sym[p:p + L].copy()
        return synth.revcomp(r) if inv else r

    for L in LENS:
        if L == 0:
            for _ in range(3):
                reads.append((np.zeros(0, np.uint8), np.zeros(0, np.uint8)))
                meta.append((0, "empty", 0, 0))
            continue
        where = {"first": CUT, "end": N_GENOME - L, "mid": P_MID, "exact": P_EXACT, "near": P_NEAR}
        for kind in KINDS:
            for inv in (0, 1):
                reads.append((take(where[kind], L, inv), _qualities(rng, L)))
                meta.append((L, kind, inv, where[kind]))
        r = take(P_N, L, 0)
        r[L // 2] = 4
        reads.append((r, _qualities(rng, L)))
        meta.append((L, "n", 0, P_N))
        for kind, p, k in (("kmax", P_KMAX, TOTALKMAX), ("over", P_OVER, TOTALKMAX + 1)):
            r = take(p, L, 0)
            for j in subst_offsets(L, k):
                r[j] = (r[j] + 1 + int(rng.integers(0, 3))) & 3
            reads.append((r, _qualities(rng, L)))
            meta.append((L, kind, 0, p))
    fill = synth.sample_reads(g, N_FILL, FILL_LEN, 0.02, seed=8, n_read_prob=0.0005)
    for i in range(N_FILL):
        reads.append((fill.bases[i * FILL_LEN:(i + 1) * FILL_LEN], _qualities(rng, FILL_LEN)))
        meta.append((FILL_LEN, "fill", int(fill.true_inv[i]), int(fill.true_pos[i])))
    order = rng.permutation(len(reads))
    reads, meta = [reads[i] for i in order], [meta[i] for i in order]
    b = _batch(reads, ids=["d%d_%s_L%d" % (i, m[1], m[0]) for i, m in enumerate(meta)])
    assert int(b.qual.max()) == 127 and b.n_reads < 450
    uniform = {L: subset(b, [i for i, m in enumerate(meta) if m[0] == L]) for L in UNIFORM}
    some = [i for i, m in enumerate(meta) if m[0] in (100, 320, 321, 2049)][:20]
    none = (np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    edge = subset(b, some)
    edge_empty = _batch([none] + [(edge.bases[int(edge.offsets[i]):int(edge.offsets[i + 1])], edge.qual[int(edge.offsets[i]):int(edge.offsets[i + 1])])
                                  for i in range(edge.n_reads)] + [none])
    # pairs: FR fragments [s, s + outer) mid-text; three per length pair and per choice of the forward mate
    m1, m2, pmeta = [], [], []
    s = 60_000
    for l1, l2 in PAIR_LENS:
        for fwd1 in (True, False, True):
            lf, lr = (l1, l2) if fwd1 else (l2, l1)
            outer = lf + PAIR_GAP + lr
            f, r = (take(s, lf, 0), _qualities(rng, lf)), (take(s + outer - lr, lr, 1), _qualities(rng, lr))
            for mate in (f, r):                                 # one substitution mid-read: sites for the pileup of the pairs
                if mate[0].shape[0] >= FILL_LEN:
                    mate[0][mate[0].shape[0] // 2] ^= 1
            m1.append(f if fwd1 else r)
            m2.append(r if fwd1 else f)
            pmeta.append((s, outer, fwd1))
            s += 7
    _W = types.SimpleNamespace(g=g, b=b, b63=twin(b), meta=meta, uniform=uniform, empty=_batch([none] * 5), edge_empty=edge_empty,
                               pairs=(_batch(m1), _batch(m2)), pair_meta=pmeta)
    return _W


def index_of(w, L: int, kind: str, inv: int = 0):
    """the read of that length, kind and strand"""
    return [i for i, m in enumerate(w.meta) if m[0] == L and m[1] == kind and m[2] == inv][0]


# ---- the oracle on the workload, once per process ------------------------------------------------------------------
_O = {}


def oracle(ora, which: str = "b", seedl: int = 32, scores: int = 1, qual: bool = True, totalkmax: int = TOTALKMAX):
    """-> namespace(info, score, ctr, hits, hoff, actr) of ora.match_unique / ora.match_all on a batch of the workload
    (`which`: "b", "b63", "empty", "edge_empty", "pairs1", "pairs2" or a uniform length); nobody may change the arrays"""
    key = (which, seedl, scores, qual, totalkmax)
    if key not in _O:
        w = workload()
        b = batch_of(w, which)
        if "g" not in _O:
            _O["g"] = ora.Genome(w.g.sym, w.g.frag_start)
        if ("ix", seedl) not in _O:
            _O[("ix", seedl)] = ora.Index(_O["g"], seedl)
        og, ix = _O["g"], _O[("ix", seedl)]
        p = ora.make_params(seedl=seedl, seedkmax=SEEDKMAX, totalkmax=totalkmax, scores=scores)
        q = b.qual if qual else None
        info, score, ctr = ora.match_unique(og, ix, p, b.bases, q, b.offsets)
        hits, hoff, actr = ora.match_all(og, ix, p, b.bases, q, b.offsets)
        for a in (info, score, hits, hoff):
            a.setflags(write=False)
        _O[key] = types.SimpleNamespace(info=info, score=score, ctr=ctr, hits=hits, hoff=hoff, actr=actr)
    return _O[key]


def batch_of(w, which):
    if isinstance(which, int):
        return w.uniform[which]
    if which in ("pairs1", "pairs2"):
        return w.pairs[int(which[-1]) - 1]
    return getattr(w, which)
