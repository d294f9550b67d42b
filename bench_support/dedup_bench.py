#!/usr/bin/env python3
"""Duplicate marking at the bench's C2 size (3 Gbp synthetic genome, 50 M x 100 bp reads, every array resident on the device):
10 % of the reads are replaced by copies of their predecessors, so that groups exist; the records come from one
real_hip_match_unique over the batch, whose time in the same run on the same build is the first yardstick; a device-to-device
copy of the records and summaries (what the marking must at least read) is the second.  Timed: real_hip_read_summary for
qualities beside byte and beside 2-bit packed bases, real_hip_mark_duplicates, and real_hip_mark_duplicates_pairs on pair
records made of the same placements (mate 2 laid 200 bases behind mate 1).  Starts nothing by itself in CI.

    python bench_support/dedup_bench.py --out profiles/dedup_bench.json

With --cli-reads N (default 2 M; 0 = skip) the `real` command line then runs on a 100 Mbp genome and N reads of 100 bases on
disk (the inputs of bench_support/cli_midsize.py), once with -sam and once with -sam -dedup 1, and the "timing:" lines of both
runs go into the file.

Times: *_kernel_ms are HIP events around the kernels (the stage's kernel_ms), *_call_ms the wall time of the synchronous call
(no copy: everything is on the device).  Minima of the steps; every step is kept.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cli_on_and_off(n_reads, G):
    """`real -sam` on files on disk without and with -dedup 1 (child processes): the stage times of both runs"""
    import subprocess
    import tempfile

    import numpy as np
    sys.path.insert(0, os.path.join(HERE, "bench_support"))
    import cli_midsize as mid
    d = tempfile.mkdtemp(prefix="real_dedup_", dir=os.environ.get("TMPDIR", "/tmp"))
    sym = np.random.default_rng(5).integers(0, 4, size=G, dtype=np.uint8)
    b, q = mid.make_reads(sym, n_reads, 100, 0.02, 6)
    fa, fq, out, sam = (os.path.join(d, x) for x in ("g.fa", "r.fq", "out.tsv", "out.sam"))
    mid.write_genome(fa, sym)
    mid.write_fastq(fq, b, q)
    base = [mid.REAL, "-t", fa, "-p", fq, "-o", out, "-e", "3", "-s", "2", "-l", "32", "-q", "1", "-sam", sam]
    res = {"reads": n_reads, "genome_bp": G, "command": "real -t g.fa -p r.fq -o out.tsv -e 3 -s 2 -l 32 -q 1 -sam out.sam [-dedup 1]", "runs": []}
    for name, extra in (("warm-up", []), ("off", []), ("on", ["-dedup", "1"])):
        t = time.time()
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        wall = time.time() - t
        err = r.stderr.decode()
        assert r.returncode == 0, err[-2000:]
        tl = [l for l in err.split("\n") if l.startswith("timing: ")][-1]
        tm = {k: float(v) for k, v in (kv.split("=") for kv in tl[len("timing: "):].split())}
        tm["process_wall_s"], tm["dedup"] = wall, name
        tm["duplicates_line"] = next((l for l in err.split("\n") if l.startswith("duplicates: ")), "")
        res["runs"].append(tm)
        print("cli", name, json.dumps(tm), flush=True)
    for f in (fa, fq, out, sam):
        os.remove(f)
    os.rmdir(d)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "dedup_bench.json"))
    ap.add_argument("--genome-mbp", type=float, default=3000.0)
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--min-qual", type=int, default=15)
    ap.add_argument("--cli-reads", type=int, default=2_000_000)
    ap.add_argument("--cli-genome-mbp", type=float, default=100.0)
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
    bv = bases.view(n, patl)
    bv[9::10] = bv[8::10][:bv[9::10].shape[0]]          # every tenth read: a copy of its predecessor (its own qualities stay)
    packed = bench.pack_bases(torch, bases, n, patl)
    info = torch.zeros(n, dtype=torch.int64, device=dev)
    score = torch.zeros(n, dtype=torch.float32, device=dev)
    result = {"genome_mbp": args.genome_mbp, "reads": n, "patl": patl, "steps": K, "min_qual": args.min_qual, "table_kind": int(m.table_kind)}

    # ---- the first yardstick: the match step of this run (2-bit packed bases, records left on the device, as the bench's headline)
    def match():
        t0 = time.perf_counter()
        m.match_unique(packed, qual, patl=patl, info=info, score=score, n_reads=n, packed=True, fresh=True)
        return (time.perf_counter() - t0) * 1e3
    match()
    for k in (rlib.K_MATCH_UNIQUE, rlib.K_MATCH_REPEAT):
        m.kernel_time(k, reset=True)
    ts = [match() for _ in range(K)]
    kms = sum(m.kernel_time(k)[0] for k in (rlib.K_MATCH_UNIQUE, rlib.K_MATCH_REPEAT)) / K
    result["match_unique"] = {"call_ms": min(ts), "call_ms_all_steps": ts, "kernel_ms_per_call": kms}
    print("match_unique", json.dumps(result["match_unique"]), flush=True)

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
                "stats": {k: st[k] for k in st if k != "kernel_ms"}}

    # ---- the summaries: the qualities are read once, 8 bytes per read are written
    sums = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    for fmt, b in (("bytes", bases), ("packed", packed)):
        r = timed(lambda: m.read_summary(b, qual, patl=patl, n_reads=n, packed=(fmt == "packed"), min_qual=args.min_qual, out=sums))
        r["gb_per_s"] = (n * patl + n * 8) / r["kernel_ms"] / 1e6
        r["kernel_over_match_kernel"] = r["kernel_ms"] / kms
        result["read_summary_%s" % fmt] = r
        print("read_summary", fmt, json.dumps(r), flush=True)

    # ---- the second yardstick: a device-to-device copy of what the marking reads (records and summaries)
    info2, sums2 = torch.empty_like(info), torch.empty_like(sums)
    cp = []
    for _ in range(K + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        info2.copy_(info)
        sums2.copy_(sums)
        e1.record()
        torch.cuda.synchronize()
        cp.append(e0.elapsed_time(e1))
    result["copy_records_and_summaries"] = {"ms": min(cp[1:]), "ms_all_steps": cp[1:], "bytes": n * 16}
    print("copy", json.dumps(result["copy_records_and_summaries"]), flush=True)
    del info2, sums2

    # ---- the marking, single-end
    dup = torch.zeros(n, dtype=torch.uint8, device=dev)
    L, h = m._L, m._h
    r = timed(lambda: m._check(L.real_hip_mark_duplicates(h, info.data_ptr(), sums.data_ptr(), n, 1, dup.data_ptr())))
    r["kernel_over_match_kernel"] = r["kernel_ms"] / kms
    r["kernel_over_copy"] = r["kernel_ms"] / result["copy_records_and_summaries"]["ms"]
    r["marked"] = int(dup.sum(dtype=torch.int64).item())
    r["checks"] = {"marked_equals_duplicates": r["marked"] == r["stats"]["duplicates"], "reads": r["stats"]["reads"] == n}
    result["mark_duplicates"] = r
    print("mark_duplicates", json.dumps(r), flush=True)

    # ---- the marking, pairs: records made of the same placements, mate 2 laid 200 bases behind mate 1 on the other strand
    state = (info >> 61) & 7
    placed = (state == 1) | (state == 2)
    pos = info & ((1 << 35) - 1)
    fwd = state == 1
    pos1, pos2 = torch.where(fwd, pos, pos + 200), torch.where(fwd, pos + 200, pos)
    words = torch.zeros((n, 5), dtype=torch.int64, device=dev)
    words[:, 2] = (pos1 & 0xffffffff) | ((pos2 & 0xffffffff) << 32)
    words[:, 4] = (((~fwd).to(torch.int64) << 8) | (placed.to(torch.int64) << 16)) << 32          # inverted1, state (Unique = 1)
    del state, placed, pos, fwd, pos1, pos2
    r = timed(lambda: m._check(L.real_hip_mark_duplicates_pairs(h, words.data_ptr(), sums.data_ptr(), sums.data_ptr(), n, 1, dup.data_ptr())))
    r["kernel_over_match_kernel"] = r["kernel_ms"] / kms
    r["marked"] = int(dup.sum(dtype=torch.int64).item())
    r["checks"] = {"marked_equals_duplicates": r["marked"] == r["stats"]["duplicates"],
                   "same_groups_as_single_end": r["stats"]["groups"] == result["mark_duplicates"]["stats"]["groups"]}
    result["mark_duplicates_pairs"] = r
    print("mark_duplicates_pairs", json.dumps(r), flush=True)
    m.close()
    del m, words, dup, sums, bases, packed, qual, info, score, sym
    torch.cuda.empty_cache()
    if args.cli_reads:
        result["cli"] = cli_on_and_off(args.cli_reads, int(args.cli_genome_mbp * 1e6))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
