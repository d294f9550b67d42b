#!/usr/bin/env python3
"""The gap rescue at the paired benches' size (3 Gbp synthetic genome, 25 M fragments of 2 x 100 bases, insert window 100..420,
arrays resident on the device).  Starts nothing by itself in CI.

    python bench_support/gap_bench.py --out profiles/gap_rescue_bench.json

A share (--indel-share) of the fragments gets an insertion of 1..3 bases into mate 2, at a random offset 8..89: the matcher
places such a mate nowhere, its fragment has no concordant pair, and mate 1 is placed on its own -- what the stage is for.  One
real_hip_match_pairs_singles leaves the final records on the device; real_hip_gap_rescue is timed on them.  Beside it, from the
same run: real_hip_match_pairs_singles itself, and the mate search (real_hip_match_pairs_search) with its kernel_ms and
positions per nanosecond -- the kernel the gap search is shaped after, which tests one diagonal per position where the gap
search tests 2 * max_gap + 1.

Times: *_kernel_ms are HIP events around the stage's kernels (its kernel_ms), *_call_ms the wall time of the synchronous
call.  Every leg records the minimum of --steps steps and keeps every step.
"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plant_insertions(torch, bases, n, patl, share, seed, dev):
    """an insertion of 1..3 random bases at a random offset 8..89 into every read of a random `share` of the batch (the read
    keeps its length: the bases behind the insertion move, the last ones fall off); -> the number of reads changed"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    idx = torch.nonzero(torch.rand(n, generator=g, device=dev) < share).reshape(-1)
    k = int(idx.shape[0])
    rd = bases.view(n, patl)[idx]
    d = torch.randint(1, 4, (k, 1), generator=g, device=dev)
    j = torch.randint(8, 90, (k, 1), generator=g, device=dev)
    col = torch.arange(patl, device=dev)[None, :]
    src = torch.where(col < j, col, torch.clamp(col - d, min=0))
    new = torch.gather(rd, 1, src)
    rnd = torch.randint(0, 4, (k, patl), generator=g, device=dev, dtype=torch.uint8)
    new = torch.where((col >= j) & (col < j + d), rnd, new)
    bases.view(n, patl)[idx] = new
    torch.cuda.synchronize()
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "gap_rescue_bench.json"))
    ap.add_argument("--genome-mbp", type=float, default=3000.0)
    ap.add_argument("--pairs", type=int, default=25_000_000)
    ap.add_argument("--indel-share", type=float, default=0.02)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "bench_support"))
    import numpy as np
    import torch
    import bench
    import pairs_bench
    from mapq_bench import timed
    from real_amd import matcher as rm
    dev = torch.device("cuda", 0)
    G, p, patl, K = int(args.genome_mbp * 1e6), args.pairs, 100, args.steps
    lo, hi = 100, 420
    opts = rm.RealOptions(seedl=32, seedkmax=2, totalkmax=3, scores=True, filter_level=2).normalise()
    sym = bench.gen_genome(torch, G, 3, dev)
    m = rm.PairMatcher(opts, device=0)
    m.set_text_symbols(0, sym, np.array([0, G], dtype=np.uint64))
    m.build_index_block()
    (b1, q1), (b2, q2) = pairs_bench.sample_pairs_device(torch, sym, p, patl, 300, 30, 0.02, 11, dev)
    del sym
    torch.cuda.empty_cache()
    planted = plant_insertions(torch, b2, p, patl, args.indel_share, 12, dev)
    result = {"genome_mbp": args.genome_mbp, "pairs": p, "patl": patl, "steps": K, "insert_window": [lo, hi], "indel_share": args.indel_share,
              "reads_with_an_insertion": planted, "table_kind": int(m.table_kind)}
    pairs, s1, s2 = (torch.zeros(p * size, dtype=torch.uint8, device=dev) for size in (40, 16, 16))
    searched = torch.zeros(p * 40, dtype=torch.uint8, device=dev)
    out = torch.zeros(p * 16, dtype=torch.uint8, device=dev)
    pp, sp = m._pair_params(lo, hi), m._search_params(0)

    def batches():
        x1, x2 = m._read_batch(b1, q1, patl=patl, n_reads=p), m._read_batch(b2, q2, patl=patl, n_reads=p)
        x1.fresh = x2.fresh = 1
        return x1, x2

    def with_singles():
        x1, x2 = batches()
        m._check(m._L.real_hip_match_pairs_singles(m._h, C.byref(x1), C.byref(x2), C.byref(pp), None, pairs.data_ptr(), s1.data_ptr(), s2.data_ptr()))

    def with_search():
        x1, x2 = batches()
        m._check(m._L.real_hip_match_pairs_search(m._h, C.byref(x1), C.byref(x2), C.byref(pp), C.byref(sp), searched.data_ptr()))
    r = timed(K, with_singles)
    result["match_pairs_singles_device_outputs"] = r
    print("match_pairs_singles", json.dumps(r), flush=True)
    r = timed(K, with_search, m.mate_search_stats)
    st = m.mate_search_stats()
    r.update(positions=st["positions"], anchors=st["anchors"], positions_per_ns=st["positions"] / (r["kernel_ms"] * 1e6))
    result["mate_search"] = r
    print("mate_search", json.dumps(r), flush=True)
    gap = dict(max_gap=8, min_flank=8, max_cost=4 * 3 + 6 + 8, margin=0)
    gp = m._gap_params(**gap)

    def rescue():
        x1, x2 = batches()
        m._check(m._L.real_hip_gap_rescue(m._h, C.byref(pp), C.byref(gp), C.byref(x1), C.byref(x2), pairs.data_ptr(), s1.data_ptr(), s2.data_ptr(), 1,
                                          out.data_ptr()))
    r = timed(K, rescue, m.gap_stats)
    st = m.gap_stats()
    searched_frags = max(1, st["eligible"] - st["skipped"])
    r.update({k: st[k] for k in ("fragments", "eligible", "other_file", "skipped", "positions", "placed", "unique", "gapped")})
    r.update(params=gap, eligible_share=st["eligible"] / p, positions_per_eligible_fragment=st["positions"] / searched_frags,
             positions_per_ns=st["positions"] / (r["kernel_ms"] * 1e6),
             diagonal_pairs_per_ns=st["positions"] * (2 * gap["max_gap"] + 1) / (r["kernel_ms"] * 1e6))
    r["positions_per_ns_over_mate_search"] = r["positions_per_ns"] / result["mate_search"]["positions_per_ns"]
    result["gap_rescue"] = r
    print("gap_rescue", json.dumps(r), flush=True)
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
