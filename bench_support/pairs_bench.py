#!/usr/bin/env python3
"""Paired-end reads at C3-like size: what a caller had to do before real_hip_match_pairs existed (two real_hip_match_all
calls with host outputs; the join on the host is not even counted) against real_hip_match_pairs, on the BASELINE genome
generator and on a genome with 5 % of its positions in 16-copy repeat families.  Starts nothing by itself in CI.

    python bench_support/pairs_bench.py --out profiles/pairs_bench.json                  # this checkout
    python bench_support/pairs_bench.py --tree /path/to/parent/checkout --out ...        # the baseline on another build

--tree: import real_amd and bench from that checkout (built) instead of this one; a checkout without PairMatcher gives
the baseline figures only.  Results are merged into --out under the key --label.  A build with the mate search adds the
search-on legs (real_hip_match_pairs_search: call time, the search kernel's own time, positions and placements per fragment,
the states with the search off and on); the leg with reads at 4 % substitutions: --errprob 0.04 --ks 5 --genomes iid.
A build with real_hip_match_pairs_all adds the legs of the enumeration of every concordant pair (outputs in pinned host
memory and left on the device, pairs per fragment, handed-over share, the kernels' own time); its comparison figure is
baseline_ms, what a caller has to do without it to see the same pairs.  --skip-search leaves the mate-search legs out.
--singles adds the legs of real_hip_match_pairs_singles (the pairs plus each mate's own placement record): the call with
pinned host outputs and with outputs left on the device, the fold's kernel time beside the join's of the same run, the
reads handed to the wave kernel, bytes downloaded, and the split of the extra time over match_pairs_ms into kernels and
download; --skip-baseline / --skip-pairs-all leave the other legs out.  --insert-hist adds the legs of
real_hip_pair_insert_hist on the records real_hip_match_pairs left on the device: the kernel's own time for the workload's
outer distances and for all records forced into one bin (n_bins 422 / 1002 / 16384), beside the time of a device-to-device copy of the same records array taken in the same run:
    python bench_support/pairs_bench.py --genomes iid --ks 3 --skip-baseline --skip-search --skip-pairs-all --insert-hist \
        --out profiles/insert_hist_bench.json  The parent's match_pairs_ms for the comparison:
the same command with --tree on a parent checkout, in the same session, alternating.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sample_pairs_device(torch, sym, n, patl, mean, sd, errprob, seed, dev, chunk=1 << 20):
    """FR mates of n fragments, on the device: fragment length ~ N(mean, sd) clipped to [patl, mean + 4 sd], uniform start,
    the forward mate is mate 1 or mate 2 by a coin flip; substitutions / qualities as bench.gen_reads"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    G = sym.shape[0]
    L = torch.clamp(torch.round(torch.randn(n, generator=g, device=dev) * sd + mean), patl, mean + 4 * sd).to(torch.int64)
    s = (torch.rand(n, generator=g, device=dev, dtype=torch.float64) * (G - L + 1).to(torch.float64)).to(torch.int64)
    fwd1 = torch.rand(n, generator=g, device=dev) < 0.5
    ar = torch.arange(patl, device=dev)
    out = []
    for is_fwd in (fwd1, ~fwd1):
        bases = torch.empty(n * patl, dtype=torch.uint8, device=dev)
        qual = torch.empty(n * patl, dtype=torch.uint8, device=dev)
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            f = is_fwd[lo:hi]
            start = torch.where(f, s[lo:hi], s[lo:hi] + L[lo:hi] - patl)
            rd = sym[start[:, None] + ar[None, :]]
            rc = torch.where(rd < 4, 3 - rd, rd).flip(1)
            rd = torch.where(f[:, None], rd, rc)
            mut = (torch.rand(rd.shape, generator=g, device=dev) < errprob) & (rd < 4)
            delta = torch.randint(1, 4, rd.shape, generator=g, device=dev, dtype=torch.uint8)
            new = torch.where(mut, (rd + delta) & 3, rd)
            bases[lo * patl:hi * patl] = new.reshape(-1)
            qual[lo * patl:hi * patl] = torch.where(mut, 9, 35).to(torch.uint8).reshape(-1)
        out.append((bases, qual))
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--label", default="this_commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "pairs_bench.json"))
    ap.add_argument("--genome-mbp", type=float, default=3000.0)
    ap.add_argument("--pairs", type=int, default=25_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--genomes", default="iid,repeat")
    ap.add_argument("--errprob", type=float, default=0.02)   # substitutions per base of the reads
    ap.add_argument("--ks", default="2,3")                   # the -e values (totalkmax) measured
    ap.add_argument("--skip-search", action="store_true")    # leave the mate-search legs out
    ap.add_argument("--skip-baseline", action="store_true")  # leave the two-match_all baseline out
    ap.add_argument("--skip-pairs-all", action="store_true") # leave the legs of the enumeration out
    ap.add_argument("--singles", action="store_true")        # add the legs of real_hip_match_pairs_singles
    ap.add_argument("--insert-hist", action="store_true")    # add the legs of real_hip_pair_insert_hist on the records left on the device
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    import numpy as np
    import torch
    import bench
    from real_amd import lib as rlib
    from real_amd import matcher as rm
    have_pairs = hasattr(rm, "PairMatcher")
    dev = torch.device("cuda", 0)
    G, n, patl, lo_ins, hi_ins = int(args.genome_mbp * 1e6), args.pairs, 100, 100, 420
    result = {"genome_mbp": args.genome_mbp, "pairs": n, "patl": patl, "insert": [lo_ins, hi_ins], "steps": args.steps, "errprob": args.errprob,
              "tree_has_match_pairs": have_pairs}
    for kind in args.genomes.split(","):
        sym = bench.gen_genome(torch, G, 3, dev)
        if kind == "repeat":                       # 5 % of the positions in families of 16 exact copies of 1 kbp (bench_support/repeat_genome.py)
            fam = int(G * 0.05 / (16 * 1000))
            gg = torch.Generator(device="cpu"); gg.manual_seed(7)
            ar = torch.arange(1000, device=dev)
            src = torch.randint(0, G - 1000, (fam,), generator=gg).to(dev)
            for c in range(15):
                dst = torch.randint(0, G - 1000, (fam,), generator=gg).to(dev)
                sym[(dst[:, None] + ar[None, :]).reshape(-1)] = sym[(src[:, None] + ar[None, :]).reshape(-1)]
        (b1, q1), (b2, q2) = sample_pairs_device(torch, sym, n, patl, 300, 30, args.errprob, 11, dev)
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        Cls = rm.PairMatcher if have_pairs else rm.HipMatcher
        m = Cls(rm.RealOptions(seedl=32, seedkmax=2, totalkmax=2, scores=True).normalise(), device=0)
        m.set_text_symbols(0, sym, np.array([0, G], dtype=np.uint64))
        m.build_index_block()
        del sym
        torch.cuda.empty_cache()
        L = m._L

        def batch(b, q):
            rb = m._batch(b, q, None, patl, n)
            rb.on_device = 2                       # read arrays on the device, outputs in host memory
            return rb
        for tk in (int(v) for v in args.ks.split(",")):
            m.set_match_params(totalkmax=tk)
            key = "%s_k%d" % (kind, tk)
            r = {}
            # -- baseline: two real_hip_match_all calls with host outputs (pinned buffers, sized by a first call)
            hits, hoff, need = None, m.host_alloc(n + 1, np.uint64), [0, 0]
            cap = int(n * 1.5)
            for attempt in range(0 if args.skip_baseline else 2):
                hits = m.host_alloc(cap, rlib.HIT_DTYPE)
                ok = True
                for j, (b, q) in enumerate(((b1, q1), (b2, q2))):
                    rb, nout = batch(b, q), C.c_uint64(0)
                    rc = L.real_hip_match_all(m._h, C.byref(rb), hits.ctypes.data, cap, C.byref(nout), hoff.ctypes.data)
                    need[j] = int(nout.value)
                    if rc == rlib.REAL_HIP_E_OVERFLOW:
                        ok = False
                    else:
                        m._check(rc)
                if ok:
                    break
                cap = max(need) + 16
            ts = []
            for _ in range(0 if args.skip_baseline else args.steps):
                t0 = time.perf_counter()
                for b, q in ((b1, q1), (b2, q2)):
                    rb, nout = batch(b, q), C.c_uint64(0)
                    m._check(L.real_hip_match_all(m._h, C.byref(rb), hits.ctypes.data, cap, C.byref(nout), hoff.ctypes.data))
                ts.append((time.perf_counter() - t0) * 1e3)
            if not args.skip_baseline:
                r["baseline_ms"], r["baseline_ms_all_steps"] = min(ts), ts
                r["hits_per_mate"] = [need[0] / n, need[1] / n]
                r["baseline_hit_bytes_downloaded"] = (need[0] + need[1]) * 16
            del hits
            if have_pairs:
                pp = m._pair_params(lo_ins, hi_ins)
                rec = m.host_alloc(n, rlib.PAIR_DTYPE)
                rec_dev = torch.empty(n * 40, dtype=torch.uint8, device=dev)

                def run(on_device, out_ptr):
                    rb1, rb2 = batch(b1, q1), batch(b2, q2)
                    rb1.on_device = rb2.on_device = on_device
                    rb1.fresh = rb2.fresh = 1
                    t0 = time.perf_counter()
                    m._check(L.real_hip_match_pairs(m._h, C.byref(rb1), C.byref(rb2), C.byref(pp), out_ptr))
                    return (time.perf_counter() - t0) * 1e3
                run(2, rec.ctypes.data)                     # warm-up: the hit buffers grow here
                for k in (rlib.K_MATCH_ALL, rlib.K_MATCH_REPEAT, rlib.K_ALL_SORT, rlib.K_PAIR, rlib.K_PAIR_WAVE):
                    m.kernel_time(k, reset=True)
                m.pair_stats(reset=True)
                ts = [run(2, rec.ctypes.data) for _ in range(args.steps)]
                r["match_pairs_ms"], r["match_pairs_ms_all_steps"] = min(ts), ts
                S = float(args.steps)
                r["split_ms_per_call"] = {"match_all_lane_kernels_both_mates": m.kernel_time(rlib.K_MATCH_ALL)[0] / S,
                                          "match_all_second_pass_and_wave_both_mates": m.kernel_time(rlib.K_MATCH_REPEAT)[0] / S,
                                          "sort_both_mates": m.kernel_time(rlib.K_ALL_SORT)[0] / S,
                                          "pair_lane_kernel": m.kernel_time(rlib.K_PAIR)[0] / S,
                                          "pair_wave_kernel": m.kernel_time(rlib.K_PAIR_WAVE)[0] / S}
                st = m.pair_stats()
                r["products_per_fragment"] = st["products"] / max(st["pairs"], 1)
                r["handed_over_share"] = st["handed_over"] / max(st["pairs"], 1)
                td = [run(1, rec_dev.data_ptr()) for _ in range(args.steps)]
                r["match_pairs_device_records_ms"] = min(td)
                r["split_ms_per_call"]["record_download_by_difference"] = min(ts) - min(td)
                state = np.bincount(rec["state"], minlength=3)
                r["states"] = {"nomatch": int(state[0]), "unique": int(state[1]), "nonunique": int(state[2])}
                r["record_bytes_downloaded"] = n * 40
                if hasattr(m, "mate_search_stats") and not args.skip_search:         # the same call with the mate search behind the join
                    sp = m._search_params(0)

                    def run_search(on_device, out_ptr):
                        rb1, rb2 = batch(b1, q1), batch(b2, q2)
                        rb1.on_device = rb2.on_device = on_device
                        rb1.fresh = rb2.fresh = 1
                        t0 = time.perf_counter()
                        m._check(L.real_hip_match_pairs_search(m._h, C.byref(rb1), C.byref(rb2), C.byref(pp), C.byref(sp), out_ptr))
                        return (time.perf_counter() - t0) * 1e3
                    run_search(2, rec.ctypes.data)
                    m.mate_search_stats(reset=True)
                    ts = [run_search(2, rec.ctypes.data) for _ in range(args.steps)]
                    ms = m.mate_search_stats()
                    r["match_pairs_search_ms"], r["match_pairs_search_ms_all_steps"] = min(ts), ts
                    r["search_kernel_ms_per_call"] = ms["kernel_ms"] / max(ms["launches"], 1)
                    r["search_per_fragment"] = {k: ms[k] / max(ms["fragments"], 1) for k in ("anchors", "positions", "placements")}
                    state = np.bincount(rec["state"], minlength=3)
                    r["states_search_on"] = {"nomatch": int(state[0]), "unique": int(state[1]), "nonunique": int(state[2])}
                if args.insert_hist and hasattr(m, "insert_hist"):       # the histogram of the outer distances of the records left on the device
                    lens = torch.full((n,), patl, dtype=torch.int32, device=dev)
                    one = rec_dev.clone()
                    w = one.view(torch.int32).view(n, 10)                 # words 4, 5: pos1, pos2; word 9: k2 | inverted1 << 8 | state << 16
                    w[:, 4] = torch.arange(n, dtype=torch.int32, device=dev)
                    w[:, 5] = w[:, 4] + (300 - patl)
                    w[:, 9] = rlib.PAIR_UNIQUE << 16
                    copy_to = torch.empty_like(rec_dev)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    reps = 10

                    def copy_ms(src):
                        e0.record(); copy_to.copy_(src); e1.record(); e1.synchronize()
                        return e0.elapsed_time(e1)
                    ih = {"reps": reps, "record_bytes": n * 40}
                    for n_bins in (hi_ins + 2, 1002, 16384):
                        hist = torch.zeros(n_bins, dtype=torch.int64, device=dev)
                        leg = {}
                        for name, src in (("workload", rec_dev), ("one_bin", one)):
                            m.insert_hist(src, lens, lens, n_bins, hist=hist, fresh=True)       # warm-up
                            copy_ms(src)
                            tk_, tc_ = [], []
                            for _ in range(reps):                       # kernel and copy alternate
                                m.insert_stats(reset=True)
                                m.insert_hist(src, lens, lens, n_bins, hist=hist, fresh=True)
                                tk_.append(m.insert_stats()["kernel_ms"])
                                tc_.append(copy_ms(src))
                            st = m.insert_stats()
                            leg[name] = {"kernel_ms": min(tk_), "kernel_ms_median": sorted(tk_)[reps // 2], "copy_d2d_ms": min(tc_),
                                         "copy_d2d_ms_median": sorted(tc_)[reps // 2], "kernel_over_copy": min(tk_) / min(tc_),
                                         "counted": st["counted"], "overflow": st["overflow"], "invalid": st["invalid"],
                                         "non_zero_bins": int((hist != 0).sum())}
                            if name == "workload":                      # the same histogram from torch
                                sv = src.view(torch.int32).view(n, 10)
                                uq = ((sv[:, 9] >> 16) & 255) == rlib.PAIR_UNIQUE
                                p1, p2 = sv[:, 4].to(torch.int64) & 0xffffffff, sv[:, 5].to(torch.int64) & 0xffffffff
                                outer = (torch.where(((sv[:, 9] >> 8) & 255) == 0, p2 - p1, p1 - p2) + patl)[uq]
                                leg[name]["equals_torch_bincount"] = bool(torch.equal(torch.bincount(outer.clamp(max=n_bins - 1), minlength=n_bins), hist))
                        leg["one_bin_over_workload"] = leg["one_bin"]["kernel_ms"] / leg["workload"]["kernel_ms"]
                        ih["n_bins_%d" % n_bins] = leg
                    r["insert_hist"] = ih
                    del one, copy_to, lens, w
                if args.singles and hasattr(m, "match_pairs_singles"):   # the pairs plus each mate's own placement record
                    sg_host = [m.host_alloc(n, rlib.SINGLE_DTYPE) for _ in range(2)]
                    sg_dev = [torch.empty(n * 16, dtype=torch.uint8, device=dev) for _ in range(2)]

                    def run_singles(on_device, out_ptr, s1_ptr, s2_ptr):
                        rb1, rb2 = batch(b1, q1), batch(b2, q2)
                        rb1.on_device = rb2.on_device = on_device
                        rb1.fresh = rb2.fresh = 1
                        t0 = time.perf_counter()
                        m._check(L.real_hip_match_pairs_singles(m._h, C.byref(rb1), C.byref(rb2), C.byref(pp), None, out_ptr, s1_ptr, s2_ptr))
                        return (time.perf_counter() - t0) * 1e3
                    plain = rec.copy()
                    run_singles(2, rec.ctypes.data, sg_host[0].ctypes.data, sg_host[1].ctypes.data)
                    r["singles_pairs_equal_match_pairs"] = bool(rec.tobytes() == plain.tobytes())
                    for k in (rlib.K_PAIR, rlib.K_PAIR_WAVE):
                        m.kernel_time(k, reset=True)
                    m.single_stats(reset=True)
                    ts = [run_singles(2, rec.ctypes.data, sg_host[0].ctypes.data, sg_host[1].ctypes.data) for _ in range(args.steps)]
                    sg = m.single_stats()
                    r["match_pairs_singles_ms"], r["match_pairs_singles_ms_all_steps"] = min(ts), ts
                    r["singles_fold_kernel_ms_per_call"] = sg["kernel_ms"] / S
                    r["singles_join_kernels_ms_per_call_same_run"] = (m.kernel_time(rlib.K_PAIR)[0] + m.kernel_time(rlib.K_PAIR_WAVE)[0]) / S
                    r["singles_handed_over_per_call"] = sg["handed_over"] / S
                    r["singles_hits_per_read"] = sg["hits"] / max(sg["reads"], 1)
                    td = [run_singles(1, rec_dev.data_ptr(), sg_dev[0].data_ptr(), sg_dev[1].data_ptr()) for _ in range(args.steps)]
                    r["match_pairs_singles_device_outputs_ms"], r["match_pairs_singles_device_outputs_ms_all_steps"] = min(td), td
                    r["singles_bytes_downloaded"] = n * (40 + 32)
                    extra = min(ts) - r["match_pairs_ms"]
                    on_dev = min(td) - r["match_pairs_device_records_ms"]
                    r["singles_extra_ms"] = {"over_match_pairs_ms": extra, "of_it_with_outputs_on_the_device": on_dev,
                                             "of_it_download_of_32_bytes_per_fragment_by_difference": extra - on_dev}
                    nm = rec["state"] == 0
                    t1, t2 = (sg_host[0]["tag"] >> 5) & 3, (sg_host[1]["tag"] >> 5) & 3
                    r["singles_of_nomatch_fragments"] = {"fragments": int(nm.sum()), "both_unique": int((nm & (t1 == 1) & (t2 == 1)).sum()),
                                                         "one_unique": int((nm & ((t1 == 1) != (t2 == 1))).sum()),
                                                         "a_nonunique_mate": int((nm & ((t1 == 2) | (t2 == 2))).sum()),
                                                         "neither_placed": int((nm & (t1 == 0) & (t2 == 0)).sum())}
                    del sg_dev
                if hasattr(m, "match_pairs_all") and not args.skip_pairs_all:           # every concordant pair instead of one record per fragment
                    poff = m.host_alloc(n + 1, np.uint64)
                    poff_dev = torch.empty(n + 1, dtype=torch.int64, device=dev)
                    pcap, need_p = int(n * 1.25), C.c_uint64(0)
                    ph = m.host_alloc(pcap, rlib.PAIR_HIT_DTYPE)

                    def run_all(on_device, out_ptr, off_ptr, may_overflow=False):
                        rb1, rb2 = batch(b1, q1), batch(b2, q2)
                        rb1.on_device = rb2.on_device = on_device
                        t0 = time.perf_counter()
                        rc = L.real_hip_match_pairs_all(m._h, C.byref(rb1), C.byref(rb2), C.byref(pp), out_ptr, pcap, C.byref(need_p), off_ptr)
                        if not (may_overflow and rc == rlib.REAL_HIP_E_OVERFLOW):
                            m._check(rc)
                        return (time.perf_counter() - t0) * 1e3
                    run_all(2, ph.ctypes.data, poff.ctypes.data, may_overflow=True)        # warm-up, and the size
                    if need_p.value > pcap:
                        pcap = int(need_p.value) + 16
                        ph = m.host_alloc(pcap, rlib.PAIR_HIT_DTYPE)
                    ph_dev = torch.empty(pcap * 32, dtype=torch.uint8, device=dev)
                    run_all(2, ph.ctypes.data, poff.ctypes.data)
                    m.pair_all_stats(reset=True)
                    ts = [run_all(2, ph.ctypes.data, poff.ctypes.data) for _ in range(args.steps)]
                    pa = m.pair_all_stats()
                    r["match_pairs_all_ms"], r["match_pairs_all_ms_all_steps"] = min(ts), ts
                    r["pairs_all_kernel_ms_per_call"] = pa["kernel_ms"] / float(args.steps)
                    r["pairs_per_fragment"] = pa["pairs_out"] / max(pa["fragments"], 1)
                    r["pairs_all_handed_over_share"] = pa["handed_over"] / max(pa["fragments"], 1)
                    per = (poff[1:] - poff[:-1])
                    r["fragments_with_two_or_more_pairs"] = int((per >= 2).sum())
                    r["pair_hit_bytes_downloaded"] = int(need_p.value) * 32 + (n + 1) * 8
                    td = [run_all(1, ph_dev.data_ptr(), poff_dev.data_ptr()) for _ in range(args.steps)]
                    r["match_pairs_all_device_outputs_ms"] = min(td)
                    r["pairs_all_download_by_difference_ms"] = min(ts) - min(td)
                    del ph_dev, poff_dev
            result[key] = r
            print(key, json.dumps(r), flush=True)
        m.close()
        del b1, q1, b2, q2
        torch.cuda.empty_cache()
    merged = {}
    if os.path.exists(args.out):
        merged = json.load(open(args.out))
    merged[args.label] = result
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(merged, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
