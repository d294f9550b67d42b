#!/usr/bin/env python3
"""The variant calls at the bench's C2 size (3 Gbp synthetic genome, 50 M x 100 bp reads, arrays resident on the device): the
records come from one real_hip_match_unique over the batch, whose time in the same run on the same build is one yardstick; the
other is the pileup's add of the same run.  On a second context that holds the text alone (the index is released first: the
pileup's accumulators take 20 bytes per base) a pileup is made and finished, and on top of it real_hip_call_begin / _add /
_finish are timed for min_qual 0 and 20 and for byte and 2-bit packed bases.  Starts nothing by itself in CI.

    python bench_support/call_bench.py --out profiles/call_bench.json

Times: *_kernel_ms are HIP events around the kernels (the stage's kernel_ms), *_call_ms the wall time of the call
(synchronous, records and reads on the device: no copy).  begin_call_ms includes the allocation of bitmap, rank array and
evidence.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "call_bench.json"))
    ap.add_argument("--genome-mbp", type=float, default=3000.0)
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=3)
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

    # ---- the pileup and the calls on top of it, on a context with the text alone
    p = rm.HipMatcher(opts, device=0)
    p.set_text_symbols(0, sym, frag)

    def timed(call, stats):
        """-> (wall ms of the call, kernel ms the stage gained by it, what the call returned)"""
        before = stats()["kernel_ms"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = call()
        wall = (time.perf_counter() - t0) * 1e3
        return wall, stats()["kernel_ms"] - before, got

    for fmt, b in (("bytes", bases), ("packed", packed)):
        for q in (0, 20):
            r = {}
            add = lambda f: f(b, qual, info, patl=patl, n_reads=n, packed=(fmt == "packed"))   # noqa: E731
            p.pileup_stats(reset=True)
            p.pileup_begin(q)
            r["pileup_add_call_ms"], r["pileup_add_kernel_ms"], _ = timed(lambda: add(p.pileup_add), p.pileup_stats)
            r["pileup_finish_call_ms"], r["pileup_finish_kernel_ms"], n_sites = timed(p.pileup_finish, p.pileup_stats)
            begins, adds = [], []
            for _ in range(K + 1):              # (the first one is the warm-up: begin starts again from zero each time)
                p.call_stats(reset=True)
                begins.append(timed(p.call_begin, p.call_stats)[:2])
                adds.append(timed(lambda: add(p.call_add), p.call_stats)[:2])
            r["begin_call_ms"], r["begin_kernel_ms"] = min(x[0] for x in begins[1:]), min(x[1] for x in begins[1:])
            r["add_call_ms"], r["add_kernel_ms"] = min(x[0] for x in adds[1:]), min(x[1] for x in adds[1:])
            r["add_call_ms_all_steps"], r["add_kernel_ms_all_steps"] = [x[0] for x in adds[1:]], [x[1] for x in adds[1:]]
            r["add_kernel_over_pileup_add_kernel"] = r["add_kernel_ms"] / r["pileup_add_kernel_ms"]
            r["add_kernel_over_match_kernel"] = r["add_kernel_ms"] / kms
            fin = [timed(lambda: p.call_finish(20, 4), p.call_stats) for _ in range(K)]
            r["finish_call_ms"], r["finish_kernel_ms"] = min(x[0] for x in fin), min(x[1] for x in fin)
            st = p.call_stats(reset=True)       # the counts of the last begin + add, the calls of the last finish
            ev = torch.zeros(max(n_sites, 1) * 32, dtype=torch.uint8, device=dev)
            n_ev = C.c_uint64(0)
            p._check(p._L.real_hip_call_evidence(p._h, ev.data_ptr(), n_sites, C.byref(n_ev), 1))
            cnt_sum = int(ev.view(torch.int32).view(-1, 8)[:n_sites, :4].sum(dtype=torch.int64))
            del ev
            r["stats"] = {k: st[k] for k in st if k != "kernel_ms"}
            r["stats"]["sites"] = n_sites
            r["checks"] = {"calls_returned": fin[-1][2] == st["calls"], "evidence_records": int(n_ev.value) == n_sites,
                           "placed_equals_unique_records": st["placed"] == n_unique, "cnt_sum_equals_site_bases": cnt_sum == st["site_bases"]}
            r["device_bytes_beside_the_pileup"] = G // 8 + G // 16 + 32 * n_sites
            result["%s_minq%d" % (fmt, q)] = r
            print(fmt, q, json.dumps(r), flush=True)
            p.call_end()
    p.pileup_end()
    p.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
