#!/usr/bin/env python3
"""The anchored gap placement of single reads at the gap bench's size (3 Gbp synthetic genome, 25 M reads of 100 bases with 2 %
substitutions, arrays resident on the device).  Starts nothing by itself in CI.

    python bench_support/gap_single_bench.py --out profiles/gap_single_bench.json

A share (--indel-share) of the reads gets an insertion of 1..3 bases at a random offset 8..89: the matcher places such a read
nowhere -- what the stage is for.  One real_hip_match_unique leaves the final info words on the device; real_hip_match_gapped
is timed on them.  Beside it, from the same run: real_hip_match_unique itself; real_hip_match_all of the sub-read batch of the
eligible reads, made here with torch (what the composite does between its own kernels); the stage's kernels (kernel_ms of
real_hip_gap_anchor_stats: select, extract, search) in positions and pairs of diagonals per nanosecond; and the gap rescue's
recorded positions per nanosecond (profiles/gap_rescue_bench.json).  The plants are known: a planted read counts as
recovered if its record is Unique with an insertion and starts within max_gap of where the read was taken from.

Times: *_kernel_ms are HIP events around the stage's kernels, *_call_ms the wall time of the synchronous call.  Every leg
records the minimum of --steps steps and keeps every step.
"""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plant_insertions(torch, bases, n, patl, share, seed, dev):
    """gap_bench.plant_insertions, keeping what was planted -> (indices of the reads changed, the insertions' lengths)"""
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
    return idx, d.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "gap_single_bench.json"))
    ap.add_argument("--genome-mbp", type=float, default=3000.0)
    ap.add_argument("--reads", type=int, default=25_000_000)
    ap.add_argument("--indel-share", type=float, default=0.02)
    ap.add_argument("--anchor", type=int, default=32)
    ap.add_argument("--anchors", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "bench_support"))
    import numpy as np
    import torch
    import bench
    from mapq_bench import timed
    from real_amd import matcher as rm
    dev = torch.device("cuda", 0)
    G, n, patl, K, A = int(args.genome_mbp * 1e6), args.reads, 100, args.steps, args.anchor
    opts = rm.RealOptions(seedl=32, seedkmax=2, totalkmax=3, scores=True, filter_level=2).normalise()
    sym = bench.gen_genome(torch, G, 3, dev)
    m = rm.AllMatcher(opts, device=0)
    m.set_text_symbols(0, sym, np.array([0, G], dtype=np.uint64))
    m.build_index_block()
    bases, qual, pos, inv = bench.gen_reads(torch, sym, n, patl, 0.02, 11, dev, shuffle=True)
    del sym
    torch.cuda.empty_cache()
    idx, d = plant_insertions(torch, bases, n, patl, args.indel_share, 12, dev)
    planted = int(idx.shape[0])
    result = {"genome_mbp": args.genome_mbp, "reads": n, "patl": patl, "steps": K, "indel_share": args.indel_share, "reads_with_an_insertion": planted,
              "anchor_len": A, "max_anchors": args.anchors, "table_kind": int(m.table_kind), "kernel_source_hash": bench.kernel_source_hash()}
    info = torch.zeros(n, dtype=torch.int64, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    r = timed(K, lambda: m.match_unique(bases, qual, patl=patl, info=info, score=score, n_reads=n, fresh=True))
    result["match_unique"] = r
    print("match_unique", json.dumps(r), flush=True)

    # the sub-read batch of the eligible reads, as the composite makes it, and matchAll of it alone
    elig = torch.nonzero((info >> 61) == 0).reshape(-1)
    n_el = int(elig.shape[0])
    rows, qrows = bases.view(n, patl)[elig], qual.view(n, patl)[elig]
    sub = torch.stack([rows[:, :A], rows[:, patl - A:]], dim=1).reshape(-1).contiguous()
    subq = torch.stack([qrows[:, :A], qrows[:, patl - A:]], dim=1).reshape(-1).contiguous()
    del rows, qrows
    cap = 4 * n_el + 1024
    hits = torch.empty(cap * 4, dtype=torch.int32, device=dev)
    hoff = torch.empty(2 * n_el + 1, dtype=torch.int64, device=dev)
    n_hits = C.c_uint64(0)

    def sub_match_all():
        b = m._read_batch(sub, subq, patl=A, n_reads=2 * n_el)
        m._check(m._L.real_hip_match_all(m._h, C.byref(b), hits.data_ptr(), cap, C.byref(n_hits), hoff.data_ptr()))
    r = timed(K, sub_match_all)
    r.update(sub_reads=2 * n_el, hits=int(n_hits.value))
    result["sub_read_match_all"] = r
    print("sub_read_match_all", json.dumps(r), flush=True)
    del sub, subq, hits, hoff
    torch.cuda.empty_cache()

    gap = dict(max_gap=8, min_flank=8, max_cost=4 * 3 + 6 + 8, margin=0)
    gp, app = m._gap_params(**gap), m._gap_anchor_params(A, args.anchors)
    out = torch.zeros(n * 16, dtype=torch.uint8, device=dev)

    def gapped():
        b = m._read_batch(bases, qual, patl=patl, n_reads=n)
        m._check(m._L.real_hip_match_gapped(m._h, C.byref(gp), C.byref(app), C.byref(b), info.data_ptr(), 1, out.data_ptr()))
    r = timed(K, gapped, m.gap_anchor_stats)
    st = m.gap_anchor_stats()
    searched = max(1, st["eligible"] - st["skipped"] - st["crowded"] - st["unanchored"])
    r.update({k: st[k] for k in st if k not in ("launches", "kernel_ms")})
    r.update(params=gap, launches=st["launches"], eligible_share=st["eligible"] / n, anchored_share=searched / max(1, st["eligible"]),
             crowded_share=st["crowded"] / max(1, st["eligible"]), placed_share=st["placed"] / max(1, st["eligible"]),
             gapped_share=st["gapped"] / max(1, st["eligible"]), positions_per_anchored_read=st["positions"] / searched,
             positions_per_ns=st["positions"] / (r["kernel_ms"] * 1e6),
             diagonal_pairs_per_ns=st["positions"] * (2 * gap["max_gap"] + 1) / (r["kernel_ms"] * 1e6),
             call_ms_without_the_kernels=r["call_ms"] - r["kernel_ms"])
    rescue = json.load(open(os.path.join(HERE, "profiles", "gap_rescue_bench.json")))["gap_rescue"]
    r["gap_rescue_recorded_positions_per_ns"] = rescue["positions_per_ns"]
    r["positions_per_ns_over_gap_rescue"] = r["positions_per_ns"] / rescue["positions_per_ns"]
    # the plants: where the oriented read starts on the text -- a reverse read loses its last d bases, the text's first d
    rec = out.view(n, 16)[idx].cpu().numpy().view(rm._lib.GAP_PLACE_DTYPE).reshape(-1)
    want = (pos[idx] + torch.where(inv[idx] != 0, d, torch.zeros_like(d))).cpu().numpy()
    state = (rec["tag"] >> 5) & 3
    near = np.abs(rec["pos"].astype(np.int64) - want) <= gap["max_gap"]
    strand = ((rec["tag"] >> 4) & 1) == inv[idx].cpu().numpy()
    r.update(planted=planted, planted_eligible=int(((info[idx] >> 61) == 0).sum().item()), planted_placed=int((state != 0).sum()),
             planted_recovered=int(((state == 1) & (rec["gap"] < 0) & near & strand).sum()),
             planted_unique_at_the_locus=int(((state == 1) & near & strand).sum()))
    r["recall"] = r["planted_recovered"] / max(1, planted)
    result["match_gapped"] = r
    print("match_gapped", json.dumps(r), flush=True)
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
