#!/usr/bin/env python3
"""The mapping quality stage at the bench's C2 size (3 Gbp synthetic genome, 50 M x 100 bp reads, arrays resident on the
device).  Starts nothing by itself in CI.

    python bench_support/mapq_bench.py --out profiles/mapq_bench.json

Single-end: one real_hip_match_all leaves the hit lists on the device; on those lists real_hip_mapq_hits is timed beside
real_hip_single_hits (the first yardstick: the fold with the same walk and a 16-byte record) in the same run; the second
yardstick is real_hip_match_unique of the same run; then real_hip_match_mapq whole (the matchAll and the fold: what `real
-mapq 1` adds to a single-end pass) and the finish real_hip_mapq on the records of that match_unique.
Paired-end, at the size of bench_support/pairs_bench.py (25 M fragments): real_hip_match_pairs_mapq beside
real_hip_match_pairs_singles, all outputs left on the device -- the difference is what the flag costs a paired run -- and
real_hip_mapq_pairs.

Times: *_kernel_ms are HIP events around the stage's kernels (its kernel_ms), *_call_ms the wall time of the synchronous
call.  Every leg records the minimum of --steps steps and keeps every step.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(steps, call, stats=None):
    """steps + 1 calls (the first one is the warm-up): wall time of each, and the stage's kernel_ms of each where it has stats"""
    wall, kern = [], []
    for _ in range(steps + 1):
        if stats:
            stats(reset=True)
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        if stats:
            kern.append(stats()["kernel_ms"])
    r = {"call_ms": min(wall[1:]), "call_ms_all_steps": wall[1:]}
    if stats:
        r.update(kernel_ms=min(kern[1:]), kernel_ms_all_steps=kern[1:])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "mapq_bench.json"))
    ap.add_argument("--genome-mbp", type=float, default=3000.0)
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--pairs", type=int, default=25_000_000)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "bench_support"))
    import numpy as np
    import torch
    import bench
    import pairs_bench
    from real_amd import lib as rlib
    from real_amd import matcher as rm
    dev = torch.device("cuda", 0)
    G, n, patl, K = int(args.genome_mbp * 1e6), args.reads, 100, args.steps
    opts = rm.RealOptions(seedl=32, seedkmax=2, totalkmax=3, scores=True, filter_level=2).normalise()
    sym = bench.gen_genome(torch, G, 3, dev)
    m = rm.PairMatcher(opts, device=0)
    m.set_text_symbols(0, sym, np.array([0, G], dtype=np.uint64))
    m.build_index_block()
    result = {"genome_mbp": args.genome_mbp, "reads": n, "pairs": args.pairs, "patl": patl, "steps": K, "table_kind": int(m.table_kind)}

    # ---- single-end: the lists of one real_hip_match_all, left on the device
    bases, qual, _, _ = bench.gen_reads(torch, sym, n, patl, 0.02, 4, dev)
    rb = m._read_batch(bases, qual, patl=patl, n_reads=n)
    hoff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    nout = C.c_uint64(0)
    hits = torch.zeros((n + n // 4 + 1024, 4), dtype=torch.int32, device=dev)
    rc = m._L.real_hip_match_all(m._h, C.byref(rb), hits.data_ptr(), hits.shape[0], C.byref(nout), hoff.data_ptr())
    if rc == rlib.REAL_HIP_E_OVERFLOW:
        hits = torch.zeros((int(nout.value), 4), dtype=torch.int32, device=dev)
        rc = m._L.real_hip_match_all(m._h, C.byref(rb), hits.data_ptr(), hits.shape[0], C.byref(nout), hoff.data_ptr())
    m._check(rc)
    n_hits = int(nout.value)
    result["hits"] = n_hits
    lens = torch.full((n,), patl, dtype=torch.int32, device=dev)
    acc = torch.zeros((n, 5), dtype=torch.int64, device=dev)
    singles = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    info = torch.zeros(n, dtype=torch.int64, device=dev)
    score = torch.zeros(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    r = timed(K, lambda: m.mapq_hits(hits, hoff, acc=acc, fresh=True), m.mapq_stats)
    st = m.mapq_stats()
    r.update(handed_over=st["handed_over"], candidates=st["candidates"], bytes_per_read_counted_beforehand=16.0 * n_hits / n + 40 + 16)
    result["mapq_hits"] = r
    print("mapq_hits", json.dumps(r), flush=True)
    r = timed(K, lambda: m.single_hits(hits, hoff, lens, singles=singles, fresh=True), m.single_stats)
    result["single_hits"] = r
    print("single_hits", json.dumps(r), flush=True)
    result["mapq_hits"]["kernel_over_single_hits_kernel"] = result["mapq_hits"]["kernel_ms"] / r["kernel_ms"]

    def unique():
        m.match_unique(bases, qual, patl=patl, info=info, score=score, n_reads=n, fresh=True)
    for k in (rlib.K_MATCH_UNIQUE, rlib.K_MATCH_REPEAT):
        m.kernel_time(k, reset=True)
    r = timed(K, unique)
    r["kernel_ms_per_call"] = sum(m.kernel_time(k)[0] for k in (rlib.K_MATCH_UNIQUE, rlib.K_MATCH_REPEAT)) / (K + 1)
    result["match_unique"] = r
    print("match_unique", json.dumps(r), flush=True)
    result["mapq_hits"]["kernel_over_match_unique_kernel"] = result["mapq_hits"]["kernel_ms"] / r["kernel_ms_per_call"]
    del hits, hoff, singles, lens
    torch.cuda.empty_cache()
    r = timed(K, lambda: m.match_mapq(bases, qual, patl=patl, n_reads=n, acc=acc, fresh=True), m.mapq_stats)
    r["call_over_match_unique_call"] = r["call_ms"] / result["match_unique"]["call_ms"]
    result["match_mapq"] = r
    print("match_mapq", json.dumps(r), flush=True)
    out = []
    r = timed(K, lambda: out.append(m.mapq(info, score, acc)), m.mapq_stats)
    q = out[-1]
    placed = q != rlib.MAPQ_NONE
    r.update(placements=int(placed.sum()), mean_mapq=float(q[placed].float().mean()), share_of_60=float((q[placed] == 60).float().mean()))
    result["mapq_finish"] = r
    print("mapq_finish", json.dumps(r), flush=True)
    del bases, qual, acc, info, score, out, q, placed
    torch.cuda.empty_cache()

    # ---- paired-end: what the three folds add to real_hip_match_pairs_singles
    p = args.pairs
    if p:
        (b1, q1), (b2, q2) = pairs_bench.sample_pairs_device(torch, sym, p, patl, 300, 30, 0.02, 11, dev)
        del sym
        torch.cuda.empty_cache()
        recs = [torch.zeros(p * size, dtype=torch.uint8, device=dev) for size in (40, 16, 16, 40, 40, 40)]

        def batches():
            return m._read_batch(b1, q1, patl=patl, n_reads=p), m._read_batch(b2, q2, patl=patl, n_reads=p)
        pp = m._pair_params(100, 420)

        def with_singles():
            x1, x2 = batches()
            x1.fresh = x2.fresh = 1
            m._check(m._L.real_hip_match_pairs_singles(m._h, C.byref(x1), C.byref(x2), C.byref(pp), None, *[t.data_ptr() for t in recs[:3]]))

        def with_mapq():
            x1, x2 = batches()
            x1.fresh = x2.fresh = 1
            m._check(m._L.real_hip_match_pairs_mapq(m._h, C.byref(x1), C.byref(x2), C.byref(pp), None, *[t.data_ptr() for t in recs]))
        a = timed(K, with_singles)
        b = timed(K, with_mapq, m.mapq_stats)
        b["extra_call_ms_over_match_pairs_singles"] = b["call_ms"] - a["call_ms"]
        result["match_pairs_singles_device_outputs"], result["match_pairs_mapq_device_outputs"] = a, b
        print("match_pairs_singles", json.dumps(a), flush=True)
        print("match_pairs_mapq", json.dumps(b), flush=True)
        out = []
        r = timed(K, lambda: out.append(m.mapq_pairs(recs[0], recs[3], recs[1], recs[2], recs[4], recs[5])), m.mapq_stats)
        q = out[-1]
        placed = q != rlib.MAPQ_NONE
        r.update(placements=int(placed.sum()), mean_mapq=float(q[placed].float().mean()))
        result["mapq_pairs_finish"] = r
        print("mapq_pairs_finish", json.dumps(r), flush=True)
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
