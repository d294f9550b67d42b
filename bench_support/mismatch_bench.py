#!/usr/bin/env python3
"""The mismatch lists at the bench's C2 size (3 Gbp synthetic genome, 50 M x 100 bp reads, arrays resident on the device):
the records come from one real_hip_match_unique over the batch, whose time in the same run on the same build is the first
yardstick; then, on a second context that holds the text alone, real_hip_pileup_add (min_qual 0) -- the kernel that does the
same walk with atomics instead of a list -- is the second yardstick, and real_hip_mismatches is timed for byte and 2-bit
packed bases, records, offsets and lists on the device.  Starts nothing by itself in CI.

    python bench_support/mismatch_bench.py --out profiles/mismatch_bench.json

With --cli-reads N (default 2 M; 0 = skip) the `real` command line then runs on a 100 Mbp genome and N reads of 100 bases on
disk (the inputs of bench_support/cli_midsize.py), once without and once with -sam, and the "timing:" lines of both runs go
into the file: the stage that grows is what -sam costs the host.

Times: *_kernel_ms are HIP events around the kernels (the stage's kernel_ms: count, scan and emit), *_call_ms the wall time
of the synchronous call (no copy: everything is on the device; the total crosses to the host between count and emit).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cli_on_and_off(n_reads, G):
    """`real` on files on disk without and with -sam (child processes): the stage times of both runs"""
    import subprocess
    import tempfile

    import numpy as np
    sys.path.insert(0, os.path.join(HERE, "bench_support"))
    import cli_midsize as mid
    d = tempfile.mkdtemp(prefix="real_sam_", dir=os.environ.get("TMPDIR", "/tmp"))
    sym = np.random.default_rng(5).integers(0, 4, size=G, dtype=np.uint8)
    b, q = mid.make_reads(sym, n_reads, 100, 0.02, 6)
    fa, fq, out, sam = (os.path.join(d, x) for x in ("g.fa", "r.fq", "out.tsv", "out.sam"))
    mid.write_genome(fa, sym)
    mid.write_fastq(fq, b, q)
    base = [mid.REAL, "-t", fa, "-p", fq, "-o", out, "-e", "3", "-s", "2", "-l", "32", "-q", "1"]
    res = {"reads": n_reads, "genome_bp": G, "command": "real -t g.fa -p r.fq -o out.tsv -e 3 -s 2 -l 32 -q 1 [-sam out.sam]", "runs": []}
    for name, extra in (("warm-up", []), ("off", []), ("on", ["-sam", sam])):
        t = time.time()
        r = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
        wall = time.time() - t
        err = r.stderr.decode()
        assert r.returncode == 0, err[-2000:]
        tl = [l for l in err.split("\n") if l.startswith("timing: ")][-1]
        tm = {k: float(v) for k, v in (kv.split("=") for kv in tl[len("timing: "):].split())}
        tm["process_wall_s"], tm["sam"] = wall, name
        tm["sam_line"] = next((l for l in err.split("\n") if l.startswith("sam: ")), "").replace(d + os.sep, "")
        if extra:
            tm["sam_bytes"] = os.path.getsize(sam)
        res["runs"].append(tm)
        print("cli", name, json.dumps(tm), flush=True)
    for f in (fa, fq, out, sam):
        os.remove(f)
    os.rmdir(d)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "mismatch_bench.json"))
    ap.add_argument("--genome-mbp", type=float, default=3000.0)
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=5)
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
    packed = bench.pack_bases(torch, bases, n, patl)
    info = torch.zeros(n, dtype=torch.int64, device=dev)
    score = torch.zeros(n, dtype=torch.float32, device=dev)
    result = {"genome_mbp": args.genome_mbp, "reads": n, "patl": patl, "steps": K, "table_kind": int(m.table_kind)}

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
    state = (info >> 61) & 7
    n_unique = int(((state == 1) | (state == 2)).sum())
    errors = int(((info >> 41) & 15)[(state == 1) | (state == 2)].sum())
    result["match_unique"] = {"call_ms": min(ts), "call_ms_all_steps": ts, "kernel_ms_per_call": kms, "unique": n_unique, "errors_of_unique": errors}
    print("match_unique", json.dumps(result["match_unique"]), flush=True)
    m.close()
    del m
    torch.cuda.empty_cache()

    p = rm.HipMatcher(opts, device=0)
    p.set_text_symbols(0, sym, frag)
    # ---- the second yardstick: the pileup's add, the same walk with atomics
    p.pileup_begin(0)
    for fmt, b in (("bytes", bases), ("packed", packed)):
        call, kern = [], []
        for _ in range(K + 1):                  # (the first one is the warm-up)
            p.pileup_stats(reset=True)
            t0 = time.perf_counter()
            p.pileup_add(b, None, info, patl=patl, n_reads=n, packed=(fmt == "packed"))
            call.append((time.perf_counter() - t0) * 1e3)
            kern.append(p.pileup_stats()["kernel_ms"])
        result["pileup_add_%s_minq0" % fmt] = {"call_ms": min(call[1:]), "kernel_ms": min(kern[1:]), "call_ms_all_steps": call[1:], "kernel_ms_all_steps": kern[1:]}
        print("pileup_add", fmt, json.dumps(result["pileup_add_%s_minq0" % fmt]), flush=True)
    p.pileup_end()
    torch.cuda.empty_cache()

    # ---- the mismatch lists: outputs allocated once, the raw entry point timed
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    nout = C.c_uint64(0)
    out = torch.zeros(1, dtype=torch.int32, device=dev)
    for fmt, b in (("bytes", bases), ("packed", packed)):
        rb = p._read_batch(b, None, patl=patl, n_reads=n, packed=fmt == "packed")
        rc = p._L.real_hip_mismatches(p._h, C.byref(rb), info.data_ptr(), out.data_ptr(), 0, C.byref(nout), off.data_ptr())
        assert rc in (rlib.REAL_HIP_OK, rlib.REAL_HIP_E_OVERFLOW), rc      # cap 0: the count alone
        total = int(nout.value)
        if out.numel() < total:
            out = torch.zeros(total, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        call, kern, count_only = [], [], []
        for _ in range(K + 1):
            p.mismatch_stats(reset=True)
            t0 = time.perf_counter()
            p._check(p._L.real_hip_mismatches(p._h, C.byref(rb), info.data_ptr(), out.data_ptr(), out.numel(), C.byref(nout), off.data_ptr()))
            call.append((time.perf_counter() - t0) * 1e3)
            st = p.mismatch_stats(reset=True)
            kern.append(st["kernel_ms"])
            p._L.real_hip_mismatches(p._h, C.byref(rb), info.data_ptr(), out.data_ptr(), 0, C.byref(nout), off.data_ptr())
            count_only.append(p.mismatch_stats(reset=True)["kernel_ms"])
        r = {"call_ms": min(call[1:]), "kernel_ms": min(kern[1:]), "count_and_scan_kernel_ms": min(count_only[1:]),
             "call_ms_all_steps": call[1:], "kernel_ms_all_steps": kern[1:], "count_and_scan_kernel_ms_all_steps": count_only[1:],
             "stats": {k: st[k] for k in st if k != "kernel_ms"}}
        r["kernel_over_match_kernel"] = r["kernel_ms"] / kms
        r["kernel_over_pileup_add_kernel"] = r["kernel_ms"] / result["pileup_add_%s_minq0" % fmt]["kernel_ms"]
        r["checks"] = {"placed_equals_unique_records": st["placed"] == n_unique, "mismatches_equal_the_records_errors": st["mismatches"] == errors,
                       "disagree": st["disagree"], "last_offset_is_the_total": int(off[-1].item()) == total == st["mismatches"]}
        result["mismatches_%s" % fmt] = r
        print("mismatches", fmt, json.dumps(r), flush=True)
    p.close()
    del p, out, off, bases, packed, qual, info, score, sym
    torch.cuda.empty_cache()
    if args.cli_reads:
        result["cli"] = cli_on_and_off(args.cli_reads, int(args.cli_genome_mbp * 1e6))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
