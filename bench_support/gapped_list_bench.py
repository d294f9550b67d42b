#!/usr/bin/env python3
"""The gapped mismatch lists at the gap bench's size (3 Gbp synthetic genome, 25 M fragments of 2 x 100 bases, insert window
100..420, 2 % of the fragments with an insertion of 1..3 bases in mate 2, arrays resident on the device).  Starts nothing by itself
in CI.

    python bench_support/gapped_list_bench.py --out profiles/gapped_list_bench.json

gap_bench.py's workload, word for word (its plant_insertions, its seeds).  One real_hip_match_pairs_singles leaves the final
records on the device, one real_hip_gap_rescue the gap records; real_hip_mismatches_gapped is timed on those records -- the
rescue's own.  Beside it, from the same run: real_hip_mismatches_pairs (the ungapped lists of the same fragments, two lists per
fragment) and real_hip_gap_rescue itself.  The list walks one placement per placed record where the rescue examines 337 starts
per eligible fragment: its call should be a small fraction of the rescue's.

Times: *_kernel_ms are HIP events around the stage's kernels (its kernel_ms: count, scan and emit), *_call_ms the wall time of the
synchronous call.  Every leg records the minimum of --steps steps and keeps every step.
"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "gapped_list_bench.json"))
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
    from gap_bench import plant_insertions
    from mapq_bench import timed
    from real_amd import lib as rlib
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
    gaps = torch.zeros(p * 16, dtype=torch.uint8, device=dev)
    pp = m._pair_params(lo, hi)

    def batches():
        x1, x2 = m._read_batch(b1, q1, patl=patl, n_reads=p), m._read_batch(b2, q2, patl=patl, n_reads=p)
        x1.fresh = x2.fresh = 1
        return x1, x2

    x1, x2 = batches()
    m._check(m._L.real_hip_match_pairs_singles(m._h, C.byref(x1), C.byref(x2), C.byref(pp), None, pairs.data_ptr(), s1.data_ptr(), s2.data_ptr()))
    gap = dict(max_gap=8, min_flank=8, max_cost=4 * 3 + 6 + 8, margin=0)
    gp = m._gap_params(**gap)

    def rescue():
        x1, x2 = batches()
        m._check(m._L.real_hip_gap_rescue(m._h, C.byref(pp), C.byref(gp), C.byref(x1), C.byref(x2), pairs.data_ptr(), s1.data_ptr(), s2.data_ptr(), 1,
                                          gaps.data_ptr()))
    r = timed(K, rescue, m.gap_stats)
    st = m.gap_stats()
    r.update({k: st[k] for k in ("fragments", "eligible", "positions", "placed", "unique", "gapped")}, params=gap)
    result["gap_rescue"] = r
    print("gap_rescue", json.dumps(r), flush=True)

    # ---- the lists: outputs allocated once from a counting call (cap 0), the raw entry points timed
    nout = C.c_uint64(0)

    def lists_leg(name, n_lists, call, stats, keys):
        off = torch.zeros(n_lists + 1, dtype=torch.int64, device=dev)
        out = torch.zeros(1, dtype=torch.int32, device=dev)
        rc = call(out, 0, off)
        assert rc in (rlib.REAL_HIP_OK, rlib.REAL_HIP_E_OVERFLOW), rc          # cap 0: the count alone
        total = int(nout.value)
        out = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        r = timed(K, lambda: m._check(call(out, total, off)), stats)
        st = stats()
        r.update({k: st[k] for k in keys}, entries=total, lists=n_lists)
        result[name] = r
        print(name, json.dumps(r), flush=True)
        del off, out
        torch.cuda.empty_cache()
        return r

    def gapped(out, cap, off):
        x1, x2 = batches()
        return m._L.real_hip_mismatches_gapped(m._h, C.byref(x1), C.byref(x2), gaps.data_ptr(), out.data_ptr(), cap, C.byref(nout), off.data_ptr())

    def ungapped(out, cap, off):
        x1, x2 = batches()
        return m._L.real_hip_mismatches_pairs(m._h, C.byref(x1), C.byref(x2), pairs.data_ptr(), s1.data_ptr(), s2.data_ptr(), out.data_ptr(), cap,
                                              C.byref(nout), off.data_ptr())
    g = lists_leg("mismatches_gapped", p, gapped, m.gapped_list_stats,
                  ("fragments", "placed", "other_file", "invalid", "aligned_bases", "mismatches", "deleted", "inserted", "on_n", "disagree", "launches"))
    u = lists_leg("mismatches_pairs", 2 * p, ungapped, m.mismatch_stats, ("reads", "placed", "bases", "mismatches", "disagree", "launches"))
    g["placed_share"] = g["placed"] / p
    g["call_ms_over_gap_rescue"] = g["call_ms"] / result["gap_rescue"]["call_ms"]
    g["call_ms_over_mismatches_pairs"] = g["call_ms"] / u["call_ms"]
    g["aligned_bases_per_ns"] = g["aligned_bases"] / (g["kernel_ms"] * 1e6)
    u["bases_per_ns"] = u["bases"] / (u["kernel_ms"] * 1e6)
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
