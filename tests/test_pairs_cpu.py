"""Paired-end reads, the parts that need no GPU: the checker against a second formulation, the fold's algebra,
sample_pairs invariants, and the ABI mirror."""
import ctypes as C
import os
import subprocess
import re

import numpy as np

from abi_header import header_structs
import pairs_checker as pc
from real_amd import lib as rlib
from real_amd import synth
from real_amd.matcher import RealOptions, new_pair_info


def _random_lists(rng, n, max_hits, scores):
    dt = np.dtype([("read", "<u8"), ("pos", "<u4"), ("frag", "<u4"), ("score", "<f4"), ("inverted", "u1"), ("k", "u1"), ("fileid", "<u2")])
    out = []
    for _ in range(2):
        cnt = rng.integers(0, max_hits + 1, size=n)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        h = np.zeros(int(off[-1]), dtype=dt)
        h["pos"] = rng.integers(0, 400, size=h.shape[0])
        h["frag"] = rng.integers(0, 2, size=h.shape[0])
        h["inverted"] = rng.integers(0, 2, size=h.shape[0])
        h["k"] = rng.integers(0, 3, size=h.shape[0])
        h["score"] = -(rng.integers(0, 5, size=h.shape[0]).astype(np.float32) * np.float32(0.7)) if scores else 1.0
        keep = []
        for i in range(n):                                 # a list holds a location once (match_all removes duplicates)
            seen = set()
            for j in range(int(off[i]), int(off[i + 1])):
                key = (int(h["pos"][j]), int(h["frag"][j]), int(h["inverted"][j]))
                if key in seen:
                    h["pos"][j] = 100_000 + j
                seen.add(key)
        out.append((h, off))
    return out


def test_checker_agrees_with_a_second_formulation():
    rng = np.random.default_rng(1)
    for scores, fm in ((True, 3 / 70.0), (True, 0.0), (False, 3 / 70.0)):
        (h1, o1), (h2, o2) = _random_lists(rng, 300, 6, scores)
        (g1, p1), (g2, p2) = _random_lists(rng, 300, 3, scores)
        l1 = rng.integers(20, 60, size=300).astype(np.uint32)
        l2 = rng.integers(20, 60, size=300).astype(np.uint32)
        files = [(0, h1, o1, h2, o2), (1, g1, p1, g2, p2)]
        a = pc.check_pairs(files, l1, l2, 40, 160, scores, fm)
        b = pc.naive_pairs(files, l1, l2, 40, 160, scores, fm)
        pc.assert_records_equal(a, b, "checker vs naive")
        assert set(np.unique(a["state"])) == {0, 1, 2}
        # the fold of the per-file records is the record of the union
        ra = pc.check_pairs(files[:1], l1, l2, 40, 160, scores, fm)
        rb = pc.check_pairs(files[1:], l1, l2, 40, 160, scores, fm)
        for order in ((ra, rb), (rb, ra)):
            m = np.array([pc.merge(order[0][i], order[1][i], pc.eps_of(scores, fm, l1[i], l2[i])) for i in range(300)], dtype=pc.REC_DTYPE)
            pc.assert_records_equal(m, a, "merge of the files")


def test_merge_is_associative_and_commutative():
    """on random states drawn from one table of locations (a location has one value wherever it appears)"""
    rng = np.random.default_rng(2)
    locs = [(int(f), int(fr), int(p), int(p) + 50, int(i)) for f, fr, p, i in
            zip(rng.integers(0, 3, 12), rng.integers(0, 2, 12), rng.integers(0, 5, 12), rng.integers(0, 2, 12))]
    locs = sorted(set(locs))
    vals = {l: float(rng.integers(-4, 0)) for l in locs}

    def state_of(subset):
        c = [(vals[l], l, (np.float32(vals[l]), np.float32(0), 1, 2)) for l in subset]
        return pc.record_of(c, 0.5)

    for _ in range(400):
        sets = [[locs[j] for j in rng.choice(len(locs), size=int(rng.integers(0, 4)), replace=False)] for _ in range(3)]
        a, b, c = (state_of(s) for s in sets)
        ab_c = pc.merge(pc.merge(a, b, 0.5), c, 0.5)
        a_bc = pc.merge(a, pc.merge(b, c, 0.5), 0.5)
        ba = pc.merge(b, a, 0.5)
        assert ab_c.tobytes() == a_bc.tobytes()
        assert pc.merge(a, b, 0.5).tobytes() == ba.tobytes()
        if not (set(sets[0]) & set(sets[1])) and not (set(sets[0]) & set(sets[2])) and not (set(sets[1]) & set(sets[2])):
            assert ab_c.tobytes() == state_of(sets[0] + sets[1] + sets[2]).tobytes()    # disjoint files: the record of the union


def test_sample_pairs_invariants():
    g, copies = synth.repeat_family_genome(300_000, 5)
    avoid = [(p, p + 760) for fam in copies for p in fam]
    loci = synth.plant_pair_repeats(g, 5, 160, 200, 6, avoid=avoid)
    assert len(loci) == 5
    for x in loci:                                       # each stretch exists exactly twice
        for lo in (x, x + 200):
            w = g.sym[lo:lo + 160]
            hits = [p for p in range(0, g.n - 160) if g.sym[p] == w[0] and np.array_equal(g.sym[p:p + 160], w)]
            assert len(hits) == 2, (x, hits)
    b1, b2 = synth.sample_pairs(g, 3000, 100, 80, 300, 30, 0.0, 7, insert_min=150, insert_max=420, copies=copies, seg_len=760,
                                rescue_loci=loci, rescue_span=160, rescue_gap=200)
    assert b1.n_reads == b2.n_reads == 3000
    cuts = np.asarray(g.frag_start[1:-1], dtype=np.int64)
    n_straddle = n_in_copy = n_rescue = n_f1 = 0
    for i in range(3000):
        mt = re.fullmatch(r"f(\d+)_(\d+)_([12])/1", b1.ids[i])
        assert mt and b2.ids[i] == b1.ids[i][:-1] + "2"
        s, L, fwd = int(mt.group(1)), int(mt.group(2)), int(mt.group(3))
        assert 150 <= L <= 420 and 0 <= s and s + L <= g.n
        fb, rb, lf, lr = (b1, b2, 100, 80) if fwd == 1 else (b2, b1, 80, 100)
        n_f1 += fwd == 1
        # FR: the forward mate is the fragment's head as it stands, the other its tail reverse-complemented
        assert not fb.true_inv[i] and rb.true_inv[i] and int(fb.true_pos[i]) == s and int(rb.true_pos[i]) == s + L - lr
        f = fb.bases[int(fb.offsets[i]):int(fb.offsets[i + 1])]
        r = rb.bases[int(rb.offsets[i]):int(rb.offsets[i + 1])]
        assert np.array_equal(f, g.sym[s:s + lf]) and np.array_equal(synth.revcomp(r), g.sym[s + L - lr:s + L])
        n_straddle += bool(((cuts > s) & (cuts < s + L)).any())
        n_in_copy += any(p <= s and s + lf <= p + 760 for p, _ in avoid)
        n_rescue += any(x <= s and s + lf <= x + 160 and x + 200 <= s + L - lr and s + L <= x + 360 for x in loci)
    assert 1000 < n_f1 < 2000 and n_straddle > 60 and n_in_copy > 300 and n_rescue > 60, (n_f1, n_straddle, n_in_copy, n_rescue)


def test_pair_abi_mirror():
    hdr = open(rlib.LIB_PATH.replace("real_amd/libreal_hip.so", "include/real_hip.h")).read()
    assert C.sizeof(rlib.RealHipPairParams) == 16 and C.sizeof(rlib.RealHipPairStats) == 32
    assert rlib.PAIR_DTYPE.itemsize == 40 and rlib.PAIR_DTYPE == pc.REC_DTYPE
    names = header_structs()["real_hip_pair"]
    assert names == list(rlib.PAIR_DTYPE.names), names
    m = re.search(r"REAL_HIP_K_PAIR = (\d+),.*?REAL_HIP_K_PAIR_WAVE = (\d+),.*?REAL_HIP_K_COUNT = (\d+)", hdr, re.S)
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (rlib.K_PAIR, rlib.K_PAIR_WAVE, 8)
    assert "#define REAL_HIP_ABI_VERSION 2" in hdr
    rec = new_pair_info(3)
    assert np.isneginf(rec["best"]).all() and np.isneginf(rec["second"]).all() and (rec["state"] == rlib.PAIR_NOMATCH).all()
    L = rlib.load()
    for s in ("real_hip_pair_hits", "real_hip_match_pairs", "real_hip_pair_stats_get"):
        assert hasattr(L, s)


def test_realoptions_paired_end_flags(tmp_path):
    """-p2 / -insert_min / -insert_max through the C++ parser (host_selftest) and the Python mirror, and their loud errors"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "real_amd", "host"), "host_selftest"], stdout=subprocess.DEVNULL)
    st = os.path.join(root, "real_amd", "host", "host_selftest")
    fq, fa = tmp_path / "m1.fq", tmp_path / "m2.fa"
    fq.write_text("@a\nACGT\n+\nIIII\n")
    fa.write_text(">a\nACGT\n")
    base = ["-t", "g.fa", "-p", str(fq), "-o", "out"]
    r = subprocess.run([st, "pair_options"] + base + ["-p2", str(fa), "-insert_min", "150", "-insert_max", "420"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split()
    assert out == [str(fa), "0", "150", "420", "1"]         # mate 2 is FASTA, mate 1 FASTQ
    out = subprocess.run([st, "pair_options"] + base, capture_output=True, text=True).stdout.split()
    assert out == [".", "0", "0", "1000", "1"]                                  # defaults, no paired-end mode
    for bad in (["-p2", str(fa), "-u", "0"], ["-p2", str(fa), "-gpus", "2"], ["-p2", str(fa), "-insert_min", "5", "-insert_max", "4"],
                ["-p2", str(tmp_path / "missing.fq")], ["-p2"]):
        r = subprocess.run([st, "pair_options"] + base + bad, capture_output=True, text=True)
        assert r.returncode != 0, bad
    assert "-p2" in subprocess.run([st, "options", "-h"], capture_output=True, text=True).stderr
    o = RealOptions.parse(base + ["-p2", "m2.fq", "-insert_min", "150", "-insert_max", "420"])
    assert (o.pattern2filename, o.insert_min, o.insert_max) == ("m2.fq", 150, 420)
    for bad in (["-u", "0"], ["-gpus", "2"], ["-insert_min", "500", "-insert_max", "420"]):
        try:
            RealOptions.parse(base + ["-p2", "m2.fq"] + bad)
        except ValueError:
            continue
        raise AssertionError(bad)
