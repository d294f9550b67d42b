#!/usr/bin/env python3
"""The pileup at the bench's C2 size (3 Gbp synthetic genome, 50 M x 100 bp reads, arrays resident on the device): the
records come from one real_hip_match_unique over the batch, whose time in the same run on the same build is the yardstick;
then, on a second context that holds the text alone (the index is released first: the accumulators take 20 bytes per base),
real_hip_pileup_begin / _add / _finish are timed for min_qual 0 and 20 and for byte and 2-bit packed bases.  Starts nothing
by itself in CI.

    python bench_support/pileup_bench.py --out profiles/pileup_bench.json

Times: *_kernel_ms are HIP events around the kernels (the stage's kernel_ms), *_call_ms the wall time of the call
(synchronous, records and reads on the device: no copy).  begin_ms is wall time and includes the allocation and the
clearing of the accumulators.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "pileup_bench.json"))
    ap.add_argument("--genome-mbp", type=float, default=3000.0)
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import bench
    from real_amd import lib as rlib
    from real_amd import matcher as rm
    dev = torch.device("cuda", 0)
    G, n, patl, K = int(args.genome_mbp * 1e6), args.reads, 100, args.steps
    opts = rm.RealOptions(seedl=32, seedkmax=2, totalkmax=3, scores=True, filter_level=2).normalise()
    frag = np.array([0, G], dtype=np.uint64)
    sym = bench.gen_genome(torch, G, 3, dev)
    m = rm.HipMatcher(opts, device=0)
    m.set_text_symbols(0, sym, frag)
    m.build_index_block()
    bases, qual, _, _ = bench.gen_reads(torch, sym, n, patl, 0.02, 4, dev)
    packed = bench.pack_bases(torch, bases, n, patl)
    info = torch.zeros(n, dtype=torch.int64, device=dev)
    score = torch.zeros(n, dtype=torch.float32, device=dev)
    result = {"genome_mbp": args.genome_mbp, "reads": n, "patl": patl, "steps": K, "table_kind": int(m.table_kind)}

    # ---- the yardstick: the match step of this run (2-bit packed bases, records left on the device, as the bench's headline)
    def match():
        t0 = time.perf_counter()
        m.match_unique(packed, qual, patl=patl, info=info, score=score, n_reads=n, packed=True, fresh=True)
        return (time.perf_counter() - t0) * 1e3
    match()
    for k in (rlib.K_MATCH_UNIQUE, rlib.K_MATCH_REPEAT):
        m.kernel_time(k, reset=True)
    ts = [match() for _ in range(K)]
    kms = sum(m.kernel_time(k)[0] for k in (rlib.K_MATCH_UNIQUE, rlib.K_MATCH_REPEAT)) / K
    state = (info >> 61) & 7
    n_unique = int(((state == 1) | (state == 2)).sum())
    result["match_unique"] = {"call_ms": min(ts), "call_ms_all_steps": ts, "kernel_ms_per_call": kms, "unique": n_unique}
    print("match_unique", json.dumps(result["match_unique"]), flush=True)
    m.close()                                   # the index goes: 20 bytes per base of accumulators come
    del m
    torch.cuda.empty_cache()

    # ---- the pileup, on a context with the text alone
    p = rm.HipMatcher(opts, device=0)
    p.set_text_symbols(0, sym, frag)

    def begin(q):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p.pileup_begin(q)
        return (time.perf_counter() - t0) * 1e3

    for fmt, b in (("bytes", bases), ("packed", packed)):
        for q in (0, 20):
            r = {"begin_ms": [begin(q)]}
            call, kern = [], []
            for _ in range(K + 1):              # (the first one is the warm-up)
                p.pileup_stats(reset=True)
                t0 = time.perf_counter()
                p.pileup_add(b, qual, info, patl=patl, n_reads=n, packed=(fmt == "packed"))
                call.append((time.perf_counter() - t0) * 1e3)
                kern.append(p.pileup_stats()["kernel_ms"])
            r["add_call_ms"], r["add_kernel_ms"] = min(call[1:]), min(kern[1:])
            r["add_call_ms_all_steps"], r["add_kernel_ms_all_steps"] = call[1:], kern[1:]
            r["add_kernel_over_match_kernel"] = r["add_kernel_ms"] / kms
            # one add, then finish: the figures of one pile
            r["begin_ms"].append(begin(q))
            p.pileup_stats(reset=True)
            p.pileup_add(b, qual, info, patl=patl, n_reads=n, packed=(fmt == "packed"))
            before = p.pileup_stats()["kernel_ms"]
            t0 = time.perf_counter()
            n_sites = p.pileup_finish()
            r["finish_call_ms"] = (time.perf_counter() - t0) * 1e3
            st = p.pileup_stats(reset=True)
            r["finish_kernel_ms"] = st["kernel_ms"] - before
            r["stats"] = {k: st[k] for k in st if k != "kernel_ms"}
            head = torch.zeros(min(1 << 24, G), dtype=torch.int32, device=dev)
            p.pileup_depth(0, head.numel(), out=head)
            r["checks"] = {"placed_equals_unique_records": st["placed"] == n_unique, "sites_returned": n_sites == st["sites"],
                           "mean_depth_of_first_16M_positions": float(head.to(torch.float64).mean()), "expected_mean_depth": st["bases"] / G}
            result["%s_minq%d" % (fmt, q)] = r
            print(fmt, q, json.dumps(r), flush=True)
    p.pileup_end()
    p.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
