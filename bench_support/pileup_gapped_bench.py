#!/usr/bin/env python3
"""The gapped placements in the pileup and the calls at the gap bench's size (3 Gbp synthetic genome, 25 M fragments of 2 x 100
bases, insert window 100..420, 2 % of the fragments with an insertion of 1..3 bases in mate 2, arrays resident on the device).
Starts nothing by itself in CI.

    python bench_support/pileup_gapped_bench.py --out profiles/pileup_gapped_bench.json

gap_bench.py's workload, word for word (its plant_insertions, its seeds).  One real_hip_match_pairs_singles leaves the final
records on the device, one real_hip_gap_rescue the gap records -- the rescue's own.  Timed on them, in one run:
real_hip_pileup_add_pairs and real_hip_pileup_add_gapped into one begun pileup, real_hip_call_add_gapped over the finished one,
and the yardstick real_hip_mismatches_gapped, whose count and emit passes walk the same records and segments.

Times: *_kernel_ms are HIP events around the stage's kernels, *_call_ms the wall time of the synchronous call.  Every leg records
the minimum of --steps steps and keeps every step.  (The adds of the steps pile up in one pileup: its counts are not the bench's
subject, its counters are per step.)
"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "pileup_gapped_bench.json"))
    ap.add_argument("--genome-mbp", type=float, default=3000.0)
    ap.add_argument("--pairs", type=int, default=25_000_000)
    ap.add_argument("--indel-share", type=float, default=0.02)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--min-qual", type=int, default=20)
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
              "reads_with_an_insertion": planted, "min_qual": args.min_qual, "table_kind": int(m.table_kind),
              "kernel_source_hash": bench.kernel_source_hash()}
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

    def leg(name, call, stats, keys):
        r = timed(K, call, stats)
        st = stats()
        r.update({k: st[k] for k in keys})
        result[name] = r
        print(name, json.dumps(r), flush=True)
        return r

    def rescue():
        x1, x2 = batches()
        m._check(m._L.real_hip_gap_rescue(m._h, C.byref(pp), C.byref(gp), C.byref(x1), C.byref(x2), pairs.data_ptr(), s1.data_ptr(), s2.data_ptr(), 1,
                                          gaps.data_ptr()))
    leg("gap_rescue", rescue, m.gap_stats, ("fragments", "eligible", "positions", "placed", "unique", "gapped"))

    # ---- the yardstick: the gapped lists of the same records (outputs allocated once from a counting call, cap 0)
    nout = C.c_uint64(0)
    off = torch.zeros(p + 1, dtype=torch.int64, device=dev)
    out = torch.zeros(1, dtype=torch.int32, device=dev)

    def gapped_lists(out, cap):
        x1, x2 = batches()
        return m._L.real_hip_mismatches_gapped(m._h, C.byref(x1), C.byref(x2), gaps.data_ptr(), out.data_ptr(), cap, C.byref(nout), off.data_ptr())
    rc = gapped_lists(out, 0)
    assert rc in (rlib.REAL_HIP_OK, rlib.REAL_HIP_E_OVERFLOW), rc
    total = int(nout.value)
    out = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    y = leg("mismatches_gapped", lambda: m._check(gapped_lists(out, total)), m.gapped_list_stats,
            ("fragments", "placed", "aligned_bases", "mismatches", "deleted", "inserted", "launches"))
    y["entries"] = total
    del off, out
    torch.cuda.empty_cache()

    # ---- the pileup: the ungapped pairs and the gapped records into one begun pileup
    gkeys = ("records", "placed", "ungapped", "aligned_bases", "deleted", "inserted", "mismatches", "low_qual", "n_dropped", "site_bases", "site_low_qual",
             "launches")
    m.pileup_begin(args.min_qual)

    def add_pairs():
        x1, x2 = batches()
        m._check(m._L.real_hip_pileup_add_pairs(m._h, C.byref(x1), C.byref(x2), pairs.data_ptr()))

    def add_gapped():
        x1, x2 = batches()
        m._check(m._L.real_hip_pileup_add_gapped(m._h, C.byref(x1), C.byref(x2), gaps.data_ptr()))

    def call_gapped():
        x1, x2 = batches()
        m._check(m._L.real_hip_call_add_gapped(m._h, C.byref(x1), C.byref(x2), gaps.data_ptr()))
    u = leg("pileup_add_pairs", add_pairs, m.pileup_stats, ("reads", "placed", "bases", "mismatches", "low_qual", "launches"))
    a = leg("pileup_add_gapped", add_gapped, m.pileup_gapped_stats, gkeys)
    result["pileup_sites"] = m.pileup_finish()
    m.call_begin()
    c = leg("call_add_gapped", call_gapped, m.pileup_gapped_stats, gkeys)
    a["placed_share"] = a["placed"] / p
    a["kernel_ms_over_mismatches_gapped"] = a["kernel_ms"] / y["kernel_ms"]
    a["kernel_ms_over_pileup_add_pairs"] = a["kernel_ms"] / u["kernel_ms"]
    a["aligned_bases_per_ns"] = a["aligned_bases"] / (a["kernel_ms"] * 1e6)
    u["bases_per_ns"] = u["bases"] / (u["kernel_ms"] * 1e6)
    c["kernel_ms_over_mismatches_gapped"] = c["kernel_ms"] / y["kernel_ms"]
    print("summary", json.dumps({k: result[k]["kernel_ms"] for k in ("gap_rescue", "mismatches_gapped", "pileup_add_pairs", "pileup_add_gapped", "call_add_gapped")}),
          flush=True)
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
