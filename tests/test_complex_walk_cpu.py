"""real_amd/csrc/complex_walk.h on the CPU: the pure parts of the paired driver's deferred walk over complex rows.

A stand-alone program (its own main, host compiler, address and undefined-behaviour sanitizers where the compiler has
them; nothing is loaded into Python) checks
  * the descriptor: every field survives pack / unpack at its extremes -- 1 and 48 entries, lanes 0 and 63, every table,
    list and strand, first entry 0 and 2^32 - 1 (the first entry is a word of its own beside the packed one);
  * the header of a complex row judged for two key groups at once (cw_header2) against a plain loop over the sixteen
    counts: every g0, g1 in 0..15, g0 == g1 included, on random 8-bit counts with 255 among them (saturation flagged
    exactly when a count up to and including the group's is 255);
  * the flat mapping (cw_flat_find): every (descriptor, entry) is the image of exactly one flat slot, for lists of 0, 1 and
    64 descriptors and totals of 0, 63, 64, 65 and capacity x 48 entries.
"""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "complex_walk.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static int check_descriptor()
{
    int fails = 0;
    const uint32_t cnts[] = {1, 2, 47, 48}, lanes[] = {0, 1, 62, 63};
    const uint32_t bases[] = {0u, 1u, 0x80000000u, 0xffffffffu};
    for (uint32_t cnt : cnts) for (uint32_t lane : lanes) for (uint32_t table = 0; table < 4; ++table)
    for (uint32_t list = 0; list < 6; ++list) for (uint32_t strand = 0; strand < 2; ++strand) for (uint32_t base : bases) {
        // the descriptor as the kernel keeps it: two words
        const uint32_t d[2] = {base, cw_pack(lane, cnt, table, list, strand)};
        if (d[0] != base || cw_lane(d[1]) != lane || cw_cnt(d[1]) != cnt || cw_table(d[1]) != table || cw_list(d[1]) != list ||
            cw_strand(d[1]) != strand || d[1] == CW_NONE) {
            printf("descriptor lane %u cnt %u table %u list %u strand %u base %x: %x\n", lane, cnt, table, list, strand, base, d[1]);
            fails++;
        }
    }
    return fails;
}

static int check_header()
{
    int fails = 0;
    for (int trial = 0; trial < 400; ++trial) {
        uint8_t c[16];
        for (int i = 0; i < 16; ++i) {
            const uint32_t x = rnd();
            // all values, with 0, 1, 254 and 255 frequent; some headers without any 255
            c[i] = (x & 7) == 0 ? 255 : (x & 7) == 1 ? 254 : (x & 7) == 2 ? 0 : (x & 7) == 3 ? 1 : (uint8_t)(x >> 8);
            if (trial % 3 == 0 && c[i] == 255) c[i] = 17;
        }
        uint32_t w[4];
        memcpy(w, c, 16); // group 0 in the low byte of w[0] (little endian, as the device)
        for (uint32_t g0 = 0; g0 < 16; ++g0) for (uint32_t g1 = 0; g1 < 16; ++g1) {
            CwGroup a, b;
            cw_header2(w, g0, g1, a, b);
            const uint32_t gs[2] = {g0, g1};
            const CwGroup *got[2] = {&a, &b};
            for (int k = 0; k < 2; ++k) {
                uint32_t off = 0, sat = 0;
                for (uint32_t i = 0; i < gs[k]; ++i) off += c[i];
                for (uint32_t i = 0; i <= gs[k]; ++i) sat |= c[i] == 255;
                if (got[k]->off != off || got[k]->cnt != c[gs[k]] || (got[k]->sat != 0) != (sat != 0)) {
                    printf("header trial %d g0 %u g1 %u group %d: off %u / %u cnt %u / %u sat %u / %u\n", trial, g0, g1, k, got[k]->off, off,
                           got[k]->cnt, (uint32_t)c[gs[k]], got[k]->sat, sat);
                    fails++;
                }
            }
        }
    }
    return fails;
}

// every (descriptor, entry) exactly once: the slots 0 .. total - 1 map to the pairs in order
static int check_flat(const std::vector<uint32_t> &cnt, const char *what)
{
    const uint32_t n = (uint32_t)cnt.size();
    std::vector<uint32_t> pre(n ? n : 1, 0u); // exactly n words (n = 0: nothing is looked up): a read past them is caught
    uint32_t total = 0;
    for (uint32_t d = 0; d < n; ++d) { pre[d] = total; total += cnt[d]; }
    std::vector<std::vector<uint32_t>> seen(n);
    for (uint32_t d = 0; d < n; ++d) seen[d].assign(cnt[d], 0u);
    int fails = 0;
    uint32_t pd = 0, pj = 0;
    for (uint32_t t = 0; t < total; ++t) {
        const uint32_t d = cw_flat_find(pre.data(), n, t);
        if (d >= n || t < pre[d] || t - pre[d] >= cnt[d]) { printf("%s: slot %u -> descriptor %u\n", what, t, d); return fails + 1; }
        const uint32_t j = t - pre[d];
        seen[d][j]++;
        if (t && !((d == pd && j == pj + 1) || (d == pd + 1 && j == 0 && pj + 1 == cnt[pd]))) { printf("%s: slot %u out of order\n", what, t); fails++; }
        pd = d; pj = j;
    }
    for (uint32_t d = 0; d < n; ++d) for (uint32_t j = 0; j < cnt[d]; ++j)
        if (seen[d][j] != 1) { printf("%s: descriptor %u entry %u seen %u times\n", what, d, j, seen[d][j]); fails++; }
    return fails;
}

static std::vector<uint32_t> spread(uint32_t n, uint32_t total) // n counts of 1 .. 48 that add up to total
{
    std::vector<uint32_t> c(n, 1u);
    uint32_t left = total - n;
    for (uint32_t d = 0; left; d = (d + 1) % n) {
        const uint32_t add = left < 48u - c[d] ? left : 48u - c[d], some = add ? 1u + rnd() % add : 0u;
        c[d] += some; left -= some;
    }
    return c;
}

int main(int argc, char **argv)
{
    const uint32_t cap = argc > 1 ? (uint32_t)atoi(argv[1]) : 64u; // the kernel's list capacity
    int fails = check_descriptor() + check_header();
    fails += check_flat({}, "no descriptor");                                   // total 0
    for (uint32_t c : {1u, 2u, 47u, 48u}) fails += check_flat({c}, "one descriptor");
    fails += check_flat(std::vector<uint32_t>(64, 1u), "64 descriptors of one entry");           // total 64
    fails += check_flat(std::vector<uint32_t>(64, 48u), "64 descriptors of 48 entries");
    fails += check_flat(std::vector<uint32_t>(cap, 48u), "capacity x 48 entries");
    for (uint32_t total : {63u, 64u, 65u}) for (uint32_t n : {2u, 3u, 7u, 33u, 63u}) {
        if (n > total) continue;
        for (int rep = 0; rep < 8; ++rep) fails += check_flat(spread(n, total), "63 / 64 / 65 entries");
    }
    fails += check_flat(spread(64, 65), "64 descriptors, 65 entries");
    for (int rep = 0; rep < 200; ++rep) {
        const uint32_t n = 1u + rnd() % 64u;
        fails += check_flat(spread(n, n + rnd() % (47u * n + 1u)), "random");
    }
    printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
"""


def _capacity():
    """CWCAP of the paired instance, from the kernel source (the flat mapping is checked at capacity x 48 entries)"""
    import re
    text = open(os.path.join(ROOT, "real_amd", "csrc", "match_kernel.hip")).read()
    m = re.search(r"CWCAP\s*=\s*(\d+)u", text)
    assert m, "CWCAP not found in match_kernel.hip"
    return int(m.group(1))


def _compile(src, exe, flags):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "real_amd", "csrc")] + flags +
                          [str(src), "-o", str(exe)], capture_output=True, text=True)


def test_complex_walk_pure_functions(tmp_path):
    src, exe = tmp_path / "complex_walk_check.cpp", tmp_path / "complex_walk_check"
    src.write_text(PROGRAM)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # the sanitizers are left out only where the compiler demonstrably has no runtimes for them: an empty program does not
    # link with them either.  Where it does, the checks must build with them.
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    have_san = _compile(probe, tmp_path / "probe", san).returncode == 0
    r = _compile(src, exe, san if have_san else [])
    print("built %s the address and undefined-behaviour sanitizers" % ("with" if have_san else "WITHOUT (no runtimes on this machine)"))
    assert r.returncode == 0, r.stderr
    cap = _capacity()
    assert 1 <= cap <= 64
    p = subprocess.run([str(exe), str(cap)], capture_output=True, text=True, timeout=120)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.strip().endswith("0 failures")


def test_header_is_hip_free():
    """(the host compiler builds it above; this pins what that relies on)"""
    text = open(os.path.join(ROOT, "real_amd", "csrc", "complex_walk.h")).read()
    assert "hip_runtime" not in text and "#include \"real_hip_internal.h\"" not in text
