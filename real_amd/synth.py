"""Seeded synthetic genomes and reads.

The reference only ships time(0)-seeded generators (randstr.cpp:27-53,
genpat.cpp:64-166); these reproduce their *distributions* reproducibly:

* genome: i.i.d. uniform ACGT (randstr.cpp), optionally with N runs and several
  fragments (FASTA records) so the N / fragment-boundary filters are exercised;
* reads: start positions uniform over n-patl+1 and sorted, strand flip p=0.5,
  per-base substitution with probability ``errprob`` to a different base, FASTQ
  quality 'D' (unchanged) / '*' (mutated) (genpat.cpp:96-157); ground truth in
  the id ``p<pos>[_inv][_<j><old><new>]...``.

Symbols are the reference's mapped alphabet: A,C,G,T -> 0..3, anything else -> 4
(acgtnMap.hpp:39-50).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

ALPHABET = "ACGTN"


@dataclass
class Genome:
    sym: np.ndarray                 # uint8 symbols 0..4, length n
    frag_start: np.ndarray          # uint64, n_frag+1 entries, last = n ("terminal", countReads.cpp:81)
    frag_names: List[str] = field(default_factory=list)

    @property
    def n(self) -> int:
        return int(self.sym.shape[0])

    @property
    def n_frag(self) -> int:
        return int(self.frag_start.shape[0]) - 1


@dataclass
class ReadBatch:
    bases: np.ndarray               # uint8 mapped symbols, concatenated
    qual: np.ndarray                # uint8 quality values (ASCII - offset), concatenated
    offsets: np.ndarray             # uint64, n_reads+1
    ids: Optional[List[str]] = None
    true_pos: Optional[np.ndarray] = None
    true_inv: Optional[np.ndarray] = None

    @property
    def n_reads(self) -> int:
        return int(self.offsets.shape[0]) - 1


def random_genome(n: int, seed: int, n_frag: int = 1, n_runs: int = 0, n_run_len: int = 7,
                  repeats: int = 0, repeat_len: int = 300) -> Genome:
    """Uniform ACGT genome.  ``n_runs`` runs of N and ``repeats`` copied segments
    (non-unique loci) can be planted; ``n_frag`` fragments of random sizes."""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 4, size=n, dtype=np.uint8)
    for _ in range(repeats):
        if n <= 2 * repeat_len:
            break
        src = int(rng.integers(0, n - repeat_len))
        dst = int(rng.integers(0, n - repeat_len))
        seg = sym[src:src + repeat_len].copy()
        # a few substitutions so that the copies differ by 0..3 bases
        for _k in range(int(rng.integers(0, 4))):
            j = int(rng.integers(0, repeat_len))
            seg[j] = (seg[j] + 1 + rng.integers(0, 3)) & 3
        sym[dst:dst + repeat_len] = seg
    for _ in range(n_runs):
        ln = int(rng.integers(1, n_run_len + 1))
        p = int(rng.integers(0, max(1, n - ln)))
        sym[p:p + ln] = 4
    if n_frag <= 1:
        starts = np.array([0, n], dtype=np.uint64)
    else:
        cuts = np.sort(rng.choice(np.arange(1, n), size=n_frag - 1, replace=False))
        starts = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
    names = [" random_%d_%d" % (n, i) for i in range(len(starts) - 1)]
    return Genome(sym=sym, frag_start=starts, frag_names=names)


def repeat_family_genome(n: int, seed: int, families: Sequence[int] = (3, 6, 30, 60), seg_len: int = 760,
                         n_frag: int = 4, n_runs: int = 6, n_run_len: int = 7):
    """Uniform ACGT genome with EXACT repeat families: for each entry c of ``families`` one random segment of ``seg_len``
    bases is planted ``c`` times (random_genome perturbs its copies).  Copies, N runs and fragment cuts lie in disjoint
    slots, so every copy is whole, N-free and inside one fragment: a read on a family of c copies has exactly c locations
    per strand.  Returns (genome, [(segment start of each copy, ...) per family])."""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 4, size=n, dtype=np.uint8)
    slot = seg_len + 16
    n_slots = n // slot
    n_copies = int(sum(families))
    assert n_slots >= n_copies + n_runs + n_frag, "genome too small for the repeat families"
    order = rng.permutation(n_slots)
    used = 0
    copies = []
    for c in families:
        at = sorted(int(s) * slot + 8 for s in order[used:used + c])
        used += c
        seg = rng.integers(0, 4, size=seg_len, dtype=np.uint8)
        for p in at:
            sym[p:p + seg_len] = seg
        copies.append(tuple(at))
    for s in order[used:used + n_runs]:                      # N runs inside slots of their own
        ln = int(rng.integers(1, n_run_len + 1))
        p = int(s) * slot + int(rng.integers(0, slot - ln))
        sym[p:p + ln] = 4
    used += n_runs
    cuts = sorted(int(s) * slot + slot // 2 for s in order[used:used + n_frag - 1])
    starts = np.array([0] + cuts + [n], dtype=np.uint64)
    names = [" families_%d_%d" % (n, i) for i in range(len(starts) - 1)]
    return Genome(sym=sym, frag_start=starts, frag_names=names), copies


_COMP = np.array([3, 2, 1, 0, 4], dtype=np.uint8)


def revcomp(mapped: np.ndarray) -> np.ndarray:
    """Pattern::computeMapped 'transposed' (Pattern.hpp:105-128, acgtnMap.hpp:58-68)."""
    return _COMP[mapped[::-1]]


def sample_reads(g: Genome, n_reads: int, patl: int, errprob: float, seed: int,
                 q_ok: int = 35, q_mut: int = 9, with_ids: bool = True,
                 n_read_prob: float = 0.0) -> ReadBatch:
    """genpat-style reads of uniform length ``patl`` (quality values already
    offset-free: 'D'-33 = 35, '*'-33 = 9)."""
    rng = np.random.default_rng(seed)
    n = g.n
    numpos = n - patl + 1
    assert numpos > 0
    pos = np.sort(rng.integers(0, numpos, size=n_reads, dtype=np.int64))
    inv = rng.integers(0, 2, size=n_reads).astype(bool)
    idx = pos[:, None] + np.arange(patl, dtype=np.int64)[None, :]
    rd = g.sym[idx]                                    # (n_reads, patl)
    rd[inv] = _COMP[rd[inv][:, ::-1]]
    mut = rng.random(size=rd.shape) < errprob
    delta = rng.integers(1, 4, size=rd.shape).astype(np.uint8)
    orig = rd.copy()
    isn = rd > 3
    rd = np.where(mut & ~isn, (rd + delta) & 3, rd).astype(np.uint8)
    if n_read_prob > 0:
        rd = np.where(rng.random(size=rd.shape) < n_read_prob, np.uint8(4), rd)
    qual = np.where(rd == orig, np.uint8(q_ok), np.uint8(q_mut)).astype(np.uint8)
    ids = None
    if with_ids:
        ids = []
        for i in range(n_reads):
            s = "p%d" % pos[i]
            if inv[i]:
                s += "_inv"
            for j in np.nonzero(rd[i] != orig[i])[0]:
                s += "_%d%s%s" % (j, ALPHABET[orig[i, j]], ALPHABET[rd[i, j]])
            ids.append(s)
    offsets = (np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(patl))
    return ReadBatch(bases=rd.reshape(-1).copy(), qual=qual.reshape(-1).copy(), offsets=offsets, ids=ids,
                     true_pos=pos.astype(np.uint64), true_inv=inv)


def near_copy_case(n: int = 300_000, seed: int = 5, patl: int = 100, seedl: int = 32):
    """One read R with three planted near-copies X, A, C: X differs from R outside the seed, A in seed segment 2, C in seed
    segment 1 (segments of seedl/4 bases), with qualities that give score(X) < score(A) < score(C), each step smaller
    than epsilon = 3/70 * patl but X -> C larger.  The reference reaches them list by list (l0: X A | l1: X C | l2: X A C |
    l3: X | l4: X A | l5: X C; matchUniqueImplementation.cpp:407-497, match.hpp:383-413): X is taken, A turns the record
    NonUnique, C is taken, the A of list 2 turns it NonUnique for good.  Delivering all events of a window at the window's
    first turn (X*6, A*3, C*3) ends Straight at C instead -- the case VERDICT r2 constructed."""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 4, size=n, dtype=np.uint8)
    R = rng.integers(0, 4, size=patl, dtype=np.uint8)
    seg = seedl // 4
    jx, ja, jc = seedl + (patl - seedl) // 2, 2 * seg + seg // 4, seg + seg // 4
    for at, j in ((n // 30, jx), (2 * (n // 30), ja), (3 * (n // 30), jc)):
        c = R.copy()
        c[j] = (c[j] + 1) & 3
        sym[at:at + patl] = c
    q = np.full(patl, 35, dtype=np.uint8)
    q[jx], q[ja], q[jc] = 6, 3, 1
    g = Genome(sym=sym, frag_start=np.array([0, n], dtype=np.uint64), frag_names=[" random_%d" % n])
    b = ReadBatch(bases=R.copy(), qual=q, offsets=np.array([0, patl], dtype=np.uint64), ids=["xac"])
    return g, b, 3 * (n // 30)


def diverged_copy_reads(g: Genome, n_reads: int, patl: int, seedl: int, seed: int, max_copies: int = 4,
                        max_subst: int = 2, q_max: int = 40) -> ReadBatch:
    """Reads with several near-copies in the genome (planted into ``g.sym`` in place): for each read a random word R,
    2..max_copies copies of it at random places, on either strand, each with 0..max_subst substitutions at random bases
    -- inside a chosen seed segment or behind the seed --, and random qualities 0..q_max for the read.  Copies of one read
    differ in WHERE they differ from it, so they are members of different lists' equal ranges and score differently:
    the class of input on which the order of the update() calls decides the record (scores on)."""
    rng = np.random.default_rng(seed)
    n = g.n
    slot = patl + 8
    n_slots = n // slot
    want = n_reads * max_copies
    assert n_slots >= want, "genome too small for the planted copies"
    slots = rng.permutation(n_slots)[:want].reshape(n_reads, max_copies)
    bases = np.empty((n_reads, patl), dtype=np.uint8)
    qual = rng.integers(0, q_max + 1, size=(n_reads, patl)).astype(np.uint8)
    seg = max(1, seedl // 4)
    for i in range(n_reads):
        R = rng.integers(0, 4, size=patl, dtype=np.uint8)
        # the read itself: as it is, or reverse-complemented (then the seed of the oriented read is the copy's tail)
        flip = rng.random() < 0.5
        bases[i] = revcomp(R) if flip else R
        for c in range(int(rng.integers(2, max_copies + 1))):
            cp = R.copy()
            for _ in range(int(rng.choice([0, 1, 1, 1, 2][:max_subst + 3]))):
                where = int(rng.integers(0, 10))
                if where < 4:
                    j = where * seg + int(rng.integers(0, seg))              # seed segment of the straight read
                elif where < 8:
                    j = patl - 1 - ((where - 4) * seg + int(rng.integers(0, seg)))    # ... of the reversed one
                else:
                    j = int(rng.integers(0, patl))
                j = min(j, patl - 1)
                cp[j] = (cp[j] + 1 + rng.integers(0, 3)) & 3
                if rng.random() < 0.8:
                    # a low quality where the copy differs: its score lies a fraction of epsilon below the exact copy's
                    qual[i, patl - 1 - j if flip else j] = rng.integers(0, 11)
            at = int(slots[i, c]) * slot
            g.sym[at:at + patl] = cp if rng.random() < 0.7 else revcomp(cp)
    offsets = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(patl)
    return ReadBatch(bases=bases.reshape(-1).copy(), qual=qual.reshape(-1).copy(), offsets=offsets,
                     ids=["d%d" % i for i in range(n_reads)])


def concat_batches(batches: Sequence[ReadBatch]) -> ReadBatch:
    """Ragged batch from several uniform-length ones."""
    bases = np.concatenate([b.bases for b in batches])
    qual = np.concatenate([b.qual for b in batches])
    offs = [np.zeros(1, dtype=np.uint64)]
    base = np.uint64(0)
    for b in batches:
        offs.append(b.offsets[1:] + base)
        base = base + b.offsets[-1]
    ids = None
    if all(b.ids is not None for b in batches):
        ids = [s for b in batches for s in b.ids]
    return ReadBatch(bases=bases, qual=qual, offsets=np.concatenate(offs).astype(np.uint64), ids=ids)


def genome_to_fasta(g: Genome, path: str, cols: int = 60) -> None:
    with open(path, "w") as f:
        for k in range(g.n_frag):
            name = g.frag_names[k] if g.frag_names else " frag%d" % k
            f.write(">" + name + "\n")
            s = "".join(ALPHABET[c] for c in g.sym[int(g.frag_start[k]):int(g.frag_start[k + 1])])
            for i in range(0, len(s), cols):
                f.write(s[i:i + cols] + "\n")


def reads_to_fastq(b: ReadBatch, path: str, offset: int = 33) -> None:
    with open(path, "w") as f:
        for i in range(b.n_reads):
            lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
            f.write("@" + (b.ids[i] if b.ids else "r%d" % i) + "\n")
            f.write("".join(ALPHABET[c] for c in b.bases[lo:hi]) + "\n+\n")
            f.write("".join(chr(int(q) + offset) for q in b.qual[lo:hi]) + "\n")


def reads_to_fasta(b: ReadBatch, path: str) -> None:
    with open(path, "w") as f:
        for i in range(b.n_reads):
            lo, hi = int(b.offsets[i]), int(b.offsets[i + 1])
            f.write(">" + (b.ids[i] if b.ids else "r%d" % i) + "\n")
            f.write("".join(ALPHABET[c] for c in b.bases[lo:hi]) + "\n")


def pack_bases(bases: np.ndarray):
    """mapped symbols (one per byte) -> the 2-bit packed form of a real_hip_batch with packed = 1: base g of the
    concatenated batch at bits 7-2(g%4)-1.. of byte g/4.  Symbols > 3 cannot be packed (they are stored as 0); the
    caller flags their reads in nflags."""
    b = np.ascontiguousarray(bases, dtype=np.uint8)
    pad = (-b.shape[0]) % 4
    if pad:
        b = np.concatenate([b, np.zeros(pad, dtype=np.uint8)])
    q = (b & 3).reshape(-1, 4)
    return ((q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]).astype(np.uint8)


def read_nflags(bases: np.ndarray, offsets: np.ndarray) -> np.ndarray:
    """bit (i%8) of byte i/8 set iff read i holds a symbol > 3"""
    n = offsets.shape[0] - 1
    bad = np.zeros(n, dtype=bool)
    idx = np.nonzero(np.asarray(bases) > 3)[0]
    if idx.size:
        bad[np.searchsorted(offsets.astype(np.int64), idx, side="right") - 1] = True
    return np.packbits(bad, bitorder="little")


def plant_pair_repeats(g: Genome, n_loci: int, span: int, gap: int, seed: int, avoid: Sequence = ()):
    """Loci where pairing rescues a fragment: for each locus x the stretch [x, x+span) is copied to one far place and
    [x+gap, x+gap+span) to another (``g.sym`` is changed in place).  A mate inside either stretch has two locations, a
    fragment with one mate in each has one concordant placement.  Sources and destinations hold no N, no fragment cut and
    nothing of ``avoid`` (a list of (start, end) ranges, e.g. the copies of repeat_family_genome).  Returns the x."""
    rng = np.random.default_rng(seed)
    n = g.n
    busy = (g.sym > 3)
    for c in g.frag_start[1:-1]:
        busy[max(0, int(c) - 1):int(c) + 1] = True
    for lo, hi in avoid:
        busy[int(lo):int(hi)] = True
    csum = np.concatenate([[0], np.cumsum(busy)])

    def free(lo, hi):
        return 0 <= lo and hi <= n and csum[hi] == csum[lo]

    loci = []
    tries = 0
    while len(loci) < n_loci and tries < 200 * n_loci:
        tries += 1
        x, da, db = (int(v) for v in rng.integers(0, n - gap - span, size=3))
        ranges = [(x, x + gap + span), (da, da + span), (db, db + span)]
        if not all(free(lo, hi) for lo, hi in ranges):
            continue
        if any(a[0] < b[1] + gap + span and b[0] < a[1] + gap + span for i, a in enumerate(ranges) for b in ranges[i + 1:]):
            continue        # (far apart: no second concordant placement)
        g.sym[da:da + span] = g.sym[x:x + span]
        g.sym[db:db + span] = g.sym[x + gap:x + gap + span]
        for lo, hi in ranges:
            busy[lo:hi] = True
        csum = np.concatenate([[0], np.cumsum(busy)])
        loci.append(x)
    return loci


def sample_pairs(g: Genome, n: int, patl1: int, patl2: int, insert_mean: float, insert_sd: float, errprob: float, seed: int,
                 insert_min: Optional[int] = None, insert_max: Optional[int] = None, straddle_frac: float = 0.05,
                 repeat_frac: float = 0.2, copies: Sequence = (), seg_len: int = 0, rescue_loci: Sequence = (),
                 rescue_span: int = 0, rescue_gap: int = 0, rescue_frac: float = 0.05, q_ok: int = 35, q_mut: int = 9,
                 with_ids: bool = True):
    """Paired-end reads in FR orientation: a fragment [s, s+L) of the genome, L ~ N(insert_mean, insert_sd) rounded and
    clipped to [insert_min, insert_max] (defaults: the longer mate .. mean + 4 sd); the forward mate is its first patl
    bases, the other mate the reverse complement of its last ones; which of mate 1 / mate 2 is the forward one is a coin
    flip.  Substitutions and qualities as sample_reads.  ``straddle_frac`` of the fragments contain a fragment cut of the
    genome, ``repeat_frac`` have their forward mate wholly inside a copy of a repeat family (``copies``: what
    repeat_family_genome returns, ``seg_len`` its segment length) with the fragment reaching out of it where it can, and
    ``rescue_frac`` sit on a locus of plant_pair_repeats (one mate in each of the two stretches).  Returns two ReadBatches;
    the ids are ``f<s>_<L>_<1|2>/<mate>`` (1|2: the forward mate), true_pos / true_inv hold each mate's own placement."""
    rng = np.random.default_rng(seed)
    N = g.n
    lo_ins = max(patl1, patl2) if insert_min is None else int(insert_min)
    hi_ins = int(round(insert_mean + 4 * insert_sd)) if insert_max is None else int(insert_max)
    assert max(patl1, patl2) <= lo_ins <= hi_ins < N
    L = np.clip(np.rint(rng.normal(insert_mean, insert_sd, size=n)), lo_ins, hi_ins).astype(np.int64)
    s = (rng.random(n) * (N - L + 1)).astype(np.int64)
    fwd1 = rng.integers(0, 2, size=n).astype(bool)                 # mate 1 is the forward mate
    kind = rng.random(n)
    pf = np.where(fwd1, patl1, patl2).astype(np.int64)             # length of the forward / of the reverse mate
    pr = np.where(fwd1, patl2, patl1).astype(np.int64)
    cuts = np.asarray(g.frag_start[1:-1], dtype=np.int64)
    edge = 0.0
    if cuts.size and straddle_frac > 0:
        sel = np.nonzero(kind < straddle_frac)[0]
        c = cuts[rng.integers(0, cuts.size, size=sel.size)]
        s[sel] = np.clip(c - 1 - (rng.random(sel.size) * (L[sel] - 1)).astype(np.int64), 0, N - L[sel])
        edge = straddle_frac
    flat = np.array([p for fam in copies for p in fam], dtype=np.int64)
    if flat.size and repeat_frac > 0 and seg_len >= max(patl1, patl2):
        sel = np.nonzero((kind >= edge) & (kind < edge + repeat_frac))[0]
        p = flat[rng.integers(0, flat.size, size=sel.size)]
        room = np.maximum(L[sel] - pf[sel] - pr[sel], 0)            # the reverse mate can start this far behind the forward one's end
        inside = rng.random(sel.size) < 0.5                         # half of them: the whole fragment inside the copy where it fits
        off_out = seg_len - pf[sel] - (rng.random(sel.size) * (room + 1)).astype(np.int64)
        off_in = (rng.random(sel.size) * np.maximum(seg_len - L[sel] + 1, 1)).astype(np.int64)
        off = np.where(inside & (L[sel] <= seg_len), off_in, np.clip(off_out, 0, seg_len - pf[sel]))
        s[sel] = np.clip(p + off, 0, N - L[sel])
        edge += repeat_frac
    if len(rescue_loci) and rescue_frac > 0 and rescue_span >= max(patl1, patl2):
        sel = np.nonzero((kind >= edge) & (kind < edge + rescue_frac))[0]
        x = np.asarray(rescue_loci, dtype=np.int64)[rng.integers(0, len(rescue_loci), size=sel.size)]
        a = (rng.random(sel.size) * (rescue_span - pf[sel] + 1)).astype(np.int64)      # forward mate inside the first stretch
        b = (rng.random(sel.size) * (rescue_span - pr[sel] + 1)).astype(np.int64)      # reverse mate inside the second
        s[sel] = x + a
        L[sel] = rescue_gap + b + pr[sel] - a
    ok = (L >= np.maximum(pf, pr)) & (L >= lo_ins) & (L <= hi_ins) & (s >= 0) & (s + L <= N)
    redo = np.nonzero(~ok)[0]                                      # (a rescue locus that cannot hold this insert: an ordinary fragment)
    L[redo] = np.clip(np.rint(insert_mean), lo_ins, hi_ins).astype(np.int64)
    s[redo] = (rng.random(redo.size) * (N - L[redo] + 1)).astype(np.int64)

    def mate(patl, is_fwd):
        start = np.where(is_fwd, s, s + L - patl)
        rd = g.sym[start[:, None] + np.arange(patl, dtype=np.int64)[None, :]]
        inv = ~is_fwd
        rd[inv] = _COMP[rd[inv][:, ::-1]]
        mut = rng.random(size=rd.shape) < errprob
        delta = rng.integers(1, 4, size=rd.shape).astype(np.uint8)
        orig = rd.copy()
        rd = np.where(mut & (rd <= 3), (rd + delta) & 3, rd).astype(np.uint8)
        qual = np.where(rd == orig, np.uint8(q_ok), np.uint8(q_mut)).astype(np.uint8)
        return rd, qual, start, inv

    out = []
    for m, (patl, is_fwd) in enumerate(((patl1, fwd1), (patl2, ~fwd1))):
        rd, qual, start, inv = mate(patl, is_fwd)
        ids = None
        if with_ids:
            ids = ["f%d_%d_%d/%d" % (s[i], L[i], 1 if fwd1[i] else 2, m + 1) for i in range(n)]
        out.append(ReadBatch(bases=rd.reshape(-1).copy(), qual=qual.reshape(-1).copy(),
                             offsets=np.arange(n + 1, dtype=np.uint64) * np.uint64(patl), ids=ids,
                             true_pos=start.astype(np.uint64), true_inv=inv))
    return out[0], out[1]


def ragged_pairs(pairs_a, pairs_b):
    """two sample_pairs results (of different read lengths) as one ragged pair of batches"""
    return concat_batches([pairs_a[0], pairs_b[0]]), concat_batches([pairs_a[1], pairs_b[1]])
