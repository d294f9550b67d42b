#!/usr/bin/env python3
"""The indel calls at the gap bench's size (3 Gbp synthetic genome, 25 M fragments of 2 x 100 bases, insert window 100..420, about
2 % of the fragments with an insertion of 1..3 bases in a mate, arrays resident on the device).  Starts nothing by itself in CI.

    python bench_support/indel_bench.py --out profiles/indel_bench.json

gap_bench.py's workload (its genome, its fragments, its seeds, its parameters), but for where the insertions come from: so that
mates show the SAME insertion and groups exist, they are planted at shared loci -- 1..3 bases are taken OUT of the text the reads
are matched against at one position in about 8200, after the fragments were sampled from the whole genome; every mate that spans
such a locus carries those bases as an insertion.  One real_hip_match_pairs_singles leaves the final records on the device, one
pileup of the Unique pairs the depth, one real_hip_gap_rescue the gap records; real_hip_indel_add and real_hip_indel_finish are
timed on those records -- the rescue's own.  Beside them, from the same run: real_hip_gap_rescue and real_hip_mismatches_gapped.

Times: *_kernel_ms are HIP events around the stage's kernels, *_call_ms the wall time of the synchronous call.  Every leg records
the minimum of --steps steps and keeps every step.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def take_out(torch, sym, every, seed, dev):
    """the text without 1..3 bases at one locus per `every` positions (at a random place of each stretch, 400 bases off its ends)
    -> (text, loci)"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    n = int(sym.shape[0])
    k = n // every
    at = torch.arange(k, device=dev) * every + 400 + torch.randint(0, every - 800, (k,), generator=g, device=dev)
    d = torch.randint(1, 4, (k,), generator=g, device=dev)
    keep = torch.ones(n, dtype=torch.bool, device=dev)
    for s in range(3):
        keep[at[d > s] + s] = False
    step = 1 << 28                                           # (a mask over more than 2^31 elements at once is beyond torch's indexing)
    return torch.cat([sym[a:a + step][keep[a:a + step]] for a in range(0, n, step)]).contiguous(), k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "indel_bench.json"))
    ap.add_argument("--genome-mbp", type=float, default=3000.0)
    ap.add_argument("--pairs", type=int, default=25_000_000)
    ap.add_argument("--locus-every", type=int, default=8200)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "bench_support"))
    import numpy as np
    import torch
    import bench
    import pairs_bench
    from mapq_bench import timed
    from real_amd import lib as rlib
    from real_amd import matcher as rm
    dev = torch.device("cuda", 0)
    G, p, patl, K = int(args.genome_mbp * 1e6), args.pairs, 100, args.steps
    lo, hi = 100, 420
    opts = rm.RealOptions(seedl=32, seedkmax=2, totalkmax=3, scores=True, filter_level=2).normalise()
    sym = bench.gen_genome(torch, G, 3, dev)
    (b1, q1), (b2, q2) = pairs_bench.sample_pairs_device(torch, sym, p, patl, 300, 30, 0.02, 11, dev)
    text, loci = take_out(torch, sym, args.locus_every, 12, dev)
    del sym
    torch.cuda.empty_cache()
    n = int(text.shape[0])
    m = rm.PairMatcher(opts, device=0)
    m.set_text_symbols(0, text, np.array([0, n], dtype=np.uint64))
    m.build_index_block()
    del text
    torch.cuda.empty_cache()
    result = {"genome_mbp": args.genome_mbp, "text_bases": n, "pairs": p, "patl": patl, "steps": K, "insert_window": [lo, hi], "loci": loci,
              "locus_every": args.locus_every, "table_kind": int(m.table_kind)}
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

    # ---- the gapped lists of the same records (outputs sized by a counting call)
    nout, off = C.c_uint64(0), torch.zeros(p + 1, dtype=torch.int64, device=dev)

    def gapped(out, cap):
        x1, x2 = batches()
        return m._L.real_hip_mismatches_gapped(m._h, C.byref(x1), C.byref(x2), gaps.data_ptr(), out.data_ptr(), cap, C.byref(nout), off.data_ptr())
    out = torch.zeros(1, dtype=torch.int32, device=dev)
    assert gapped(out, 0) in (rlib.REAL_HIP_OK, rlib.REAL_HIP_E_OVERFLOW)
    total = int(nout.value)
    out = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
    r = timed(K, lambda: m._check(gapped(out, total)), m.gapped_list_stats)
    r.update(entries=total)
    result["mismatches_gapped"] = r
    print("mismatches_gapped", json.dumps(r), flush=True)
    del out, off
    torch.cuda.empty_cache()

    # ---- the pileup the stage sits on (once), then begin + add and finish, timed apart
    m.pileup_begin(20)
    x1, x2 = batches()
    m._check(m._L.real_hip_pileup_add_pairs(m._h, C.byref(x1), C.byref(x2), pairs.data_ptr()))
    result["pileup_sites"] = m.pileup_finish()
    prm = rlib.sized(rlib.RealHipIndelParams, min_call_qual=20, min_alt=2, min_depth=4)
    n_ev, n_calls = C.c_uint64(0), C.c_uint64(0)
    adds, fins, agains = [], [], []
    for _ in range(K + 1):                                   # (the first one is the warm-up: begin starts again from zero each time)
        legs = []
        m.indel_begin()
        for call in (lambda: m._check(m._L.real_hip_indel_add(m._h, C.byref(x1), C.byref(x2), gaps.data_ptr())),
                     lambda: m._check(m._L.real_hip_indel_finish(m._h, C.byref(prm), C.byref(n_ev), C.byref(n_calls))),
                     lambda: m._check(m._L.real_hip_indel_finish(m._h, C.byref(prm), C.byref(n_ev), C.byref(n_calls)))):
            m.indel_stats(reset=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            legs.append(((time.perf_counter() - t0) * 1e3, m.indel_stats()["kernel_ms"]))
        adds.append(legs[0]); fins.append(legs[1]); agains.append(legs[2])
    m.indel_stats(reset=True)
    m.indel_begin()
    m._check(m._L.real_hip_indel_add(m._h, C.byref(x1), C.byref(x2), gaps.data_ptr()))
    m._check(m._L.real_hip_indel_finish(m._h, C.byref(prm), C.byref(n_ev), C.byref(n_calls)))
    st = m.indel_stats()
    for name, legs in (("indel_add", adds), ("indel_finish", fins), ("indel_finish_again", agains)):
        r = {"call_ms": min(x[0] for x in legs[1:]), "kernel_ms": min(x[1] for x in legs[1:]), "call_ms_all_steps": [x[0] for x in legs[1:]],
             "kernel_ms_all_steps": [x[1] for x in legs[1:]]}
        r["call_ms_over_gap_rescue"] = r["call_ms"] / result["gap_rescue"]["call_ms"]
        r["kernel_ms_over_gap_rescue"] = r["kernel_ms"] / result["gap_rescue"]["kernel_ms"]
        result[name] = r
        print(name, json.dumps(r), flush=True)
    result["indel_stats"] = {k: st[k] for k in st if k != "kernel_ms"}
    ev = m.indel_events()
    result["group_sizes"] = {str(k): int((ev["alt_n"] == k).sum()) for k in range(1, 9)}
    result["largest_group"] = int(ev["alt_n"].max()) if ev.shape[0] else 0
    print("indel_stats", json.dumps(result["indel_stats"]), json.dumps(result["group_sizes"]), flush=True)
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
