#!/usr/bin/env python3
"""The joint duplicate marking (real_hip_mark_duplicates_gapped) beside real_hip_mark_duplicates at the size of
bench_support/dedup_bench.py: 50 M records of reads of 100 bases over 3 Gbp, every tenth one a copy of its predecessor, every
array resident on the device.  The marking needs neither text nor index, so the records are made here (uniform positions, both
strands, 4 % of the reads placed nowhere) and no matcher runs.  For each share -- 0 %, 2 % and 16 %, what DESIGN 7k reports for
gapped and eligible reads -- that share of the placed records is moved from its info word to a Unique gap record of the same
placement (gap 0, so that the keys, the groups and the marks stay what they were: checked), and in the same run, on the same n,
both calls are timed.  The sibling call is the yardstick: the same sort of n keys of 64 bits; the key kernel reads 16 more bytes
for every read the info word does not place.  Starts nothing by itself in CI.

    python bench_support/dedup_gapped_bench.py --out profiles/dedup_gapped_bench.json

Times: kernel_ms are HIP events around the kernels (the stage's kernel_ms), call_ms the wall time of the synchronous call (no
copy: everything is on the device).  Minima of five steps; every step is kept.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "dedup_gapped_bench.json"))
    ap.add_argument("--genome-mbp", type=float, default=3000.0)
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--shares", default="0,2,16")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    from real_amd import matcher as rm
    dev = torch.device("cuda", 0)
    G, n, patl, K = int(args.genome_mbp * 1e6), args.reads, 100, args.steps
    m = rm.HipMatcher(rm.RealOptions(seedl=32, seedkmax=2, totalkmax=3, scores=True, filter_level=2).normalise(), device=0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    pos = torch.randint(0, G - patl, (n,), generator=gen, device=dev, dtype=torch.int64)
    state = torch.randint(1, 3, (n,), generator=gen, device=dev, dtype=torch.int64)
    state[torch.rand(n, generator=gen, device=dev) < 0.04] = 0
    info0 = (state << 61) | pos
    info0[9::10] = info0[8::10][:info0[9::10].shape[0]]          # every tenth read: a copy of its predecessor
    sums = torch.empty((n, 2), dtype=torch.int32, device=dev)
    sums[:, 0] = patl
    sums[:, 1] = torch.randint(2500, 4000, (n,), generator=gen, device=dev, dtype=torch.int32)
    del pos, state
    dup = torch.zeros(n, dtype=torch.uint8, device=dev)
    L, h = m._L, m._h
    result = {"genome_mbp": args.genome_mbp, "reads": n, "patl": patl, "steps": K, "shares": []}

    def timed(call):
        """K + 1 calls (the first one is the warm-up) -> minima and all steps of call and kernel time, the last statistics"""
        wall, kern, st = [], [], None
        for _ in range(K + 1):
            m.dup_stats(reset=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
            st = m.dup_stats(reset=True)
            kern.append(st["kernel_ms"])
        return {"call_ms": min(wall[1:]), "kernel_ms": min(kern[1:]), "call_ms_all_steps": wall[1:], "kernel_ms_all_steps": kern[1:],
                "stats": {k: st[k] for k in st if k != "kernel_ms"}, "marked": int(dup.sum(dtype=torch.int64).item())}

    base = timed(lambda: m._check(L.real_hip_mark_duplicates(h, info0.data_ptr(), sums.data_ptr(), n, 1, dup.data_ptr())))
    base_dup = dup.clone()
    result["mark_duplicates_all_info_words"] = base
    print("mark_duplicates", json.dumps(base), flush=True)
    for share in [float(x) for x in args.shares.split(",")]:
        st = (info0 >> 61) & 7
        placed = (st == 1) | (st == 2)
        move = placed & (torch.rand(n, generator=gen, device=dev) < share / 100.0)
        info = torch.where(move, torch.zeros_like(info0), info0)
        # the gap record as two 64-bit words: pos | (tag << 56), and split = gap = k = cost = 0, second = none (0xffff)
        tag = torch.where(move, (((st == 2).to(torch.int64) << 4) | (1 << 5)), torch.zeros_like(st))
        gaps = torch.empty((n, 2), dtype=torch.int64, device=dev)
        gaps[:, 0] = torch.where(move, info0 & 0xffffffff, torch.zeros_like(info0)) | (tag << 56)
        gaps[:, 1] = -(1 << 48)                  # (0xffff in the top 16 bits)
        moved = int(move.sum().item())
        del st, placed, move, tag
        sib = timed(lambda: m._check(L.real_hip_mark_duplicates(h, info.data_ptr(), sums.data_ptr(), n, 1, dup.data_ptr())))
        joint = timed(lambda: m._check(L.real_hip_mark_duplicates_gapped(h, info.data_ptr(), gaps.data_ptr(), sums.data_ptr(), n, 1, dup.data_ptr())))
        r = {"share_percent": share, "moved_to_gap_records": moved, "mark_duplicates": sib, "mark_duplicates_gapped": joint,
             "kernel_ratio": joint["kernel_ms"] / sib["kernel_ms"], "call_ratio": joint["call_ms"] / sib["call_ms"],
             "checks": {"marks_are_those_of_all_info_words": bool(torch.equal(dup, base_dup)),
                        "stats_are_those_of_all_info_words": all(joint["stats"][k] == base["stats"][k] for k in ("reads", "placed", "groups", "duplicates")),
                        "launches": joint["stats"]["launches"] == 3}}
        result["shares"].append(r)
        print("share", json.dumps(r), flush=True)
        del info, gaps
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
