#!/usr/bin/env python3
"""Randomised campaign over the placement stages: the chains of tests/stage_fuzz.py (matcher, pair join / singles / mate search,
every-pair enumeration, insert histogram, MAPQ, duplicates, mismatch lists, gap rescue / anchored gap placement, gapped lists,
pileup, SNP calls, indel calls) on configuration after configuration, the device against the checkers.  Not part of the test
suite (run time is open-ended); prints `DIFF <stage> <cfg>` for every configuration that differs, a summary line, and exits 1 if
any did.  Unlike fuzz_parity.py it STOPS AT THE FIRST EXCEPTION: a configuration the library refuses is a bug of the generator,
and after a device error nothing more may run on the GPU in this process.

    python bench_support/fuzz_stages.py [--seconds 300] [--seed 1000] [--kind paired|single|both] [--only SEED ...]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300)
    ap.add_argument("--seed", type=int, default=1000, help="the first seed; the campaign counts up from it")
    ap.add_argument("--kind", choices=("paired", "single", "both"), default="both")
    ap.add_argument("--only", type=int, nargs="*", default=[], help="run exactly these seeds (of --kind) and stop")
    args = ap.parse_args()
    import torch
    torch.cuda.init()       # (before the library opens its own contexts: afterwards torch finds no device in this process)
    torch.zeros(1, device="cuda")
    import oracle_lib as ora
    ora.build()
    import stage_fuzz as sf
    kinds = ("paired", "single") if args.kind == "both" else (args.kind,)
    t0 = time.time()
    done = bad = 0
    seed = args.seed
    todo = list(args.only)
    while (todo or not args.only) and (args.only or time.time() - t0 < args.seconds):
        s = todo.pop(0) if args.only else seed
        seed += 1
        for kind in kinds:
            cfg = sf.draw(kind, s)
            try:
                sf.run(cfg, ora)                      # (any other exception ends the campaign: see above)
            except sf.StageDiff as e:
                bad += 1
                print("DIFF", e.stage, repr(cfg), "|", str(e)[-300:].replace("\n", " "), flush=True)
            except BaseException:
                print("EXC", repr(cfg), flush=True)
                raise
            else:
                if done % 10 == 0:
                    print("ok  ", kind, s, "%.0f s" % (time.time() - t0), flush=True)
            done += 1
            sf._WORK.clear()                          # (a campaign does not keep what it will not meet again)
            sf._EXPECTED.clear()
    print("fuzz_stages: %d configurations, %d differ" % (done, bad), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
