"""real_amd/csrc/row_bytes.h on the CPU: the byte addresses the paired driver reads a simple row's keys and positions at.

A stand-alone program (its own main, host compiler, address and undefined-behaviour sanitizers where the compiler has
them) fills a row with distinct bytes, swizzles it the way the transpose of match_rows_paired does -- piece p of a lane's
row at piece p ^ (lane & 7) -- and compares, for every entry 0..19 and every swizzle 0..7, what the new helpers read with
the formulation they replace: halfword rh_row_entry_hw(j) = 4 + 3 j of the row, dwords fetched through the row() swizzle
((d >> 2) ^ sw) << 4 | (d & 3) << 2, the key picked as a half of one dword and the position assembled from two.
"""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "row_bytes.h"

// the formulation of real_hip_internal.h / match_kernel.hip that the helpers replace
static uint32_t entry_hw(uint32_t j) { return 4 + 3 * j; }
static uint32_t row_dword(const uint8_t *lds, uint32_t sw, uint32_t d)
{
    uint32_t v;
    memcpy(&v, lds + ((((d >> 2) ^ sw) << 4) | ((d & 3) << 2)), 4);
    return v;
}
static uint32_t rd16(const uint8_t *lds, uint32_t at, int *bad)
{
    if ((at & 1) || at + 2 > 128) { *bad = 1; return 0; }
    uint16_t v;
    memcpy(&v, lds + at, 2);
    return v;
}

int main()
{
    int fails = 0;
    uint8_t row[128], lds[128];
    for (uint32_t fill = 0; fill < 2; ++fill) {
        for (uint32_t i = 0; i < 128; ++i) row[i] = (uint8_t)(fill ? 255 - i : i + 1); // distinct bytes
        for (uint32_t sw = 0; sw < 8; ++sw) {
            for (uint32_t p = 0; p < 8; ++p) memcpy(lds + ((p ^ sw) << 4), row + (p << 4), 16);
            for (uint32_t j = 0; j < 20; ++j) {
                const uint32_t h = entry_hw(j);
                const uint32_t d0 = row_dword(lds, sw, h >> 1), d1 = row_dword(lds, sw, (h >> 1) + 1);
                const uint32_t key = (h & 1) ? (d0 >> 16) : (d0 & 0xffffu);
                const uint32_t pos = (h & 1) ? d1 : ((d0 >> 16) | (d1 << 16));
                int bad = 0;
                const uint32_t kb = rh_row_key_byte(j), p0 = rh_row_pos_byte(j, 0), p1 = rh_row_pos_byte(j, 1);
                // addresses: the bytes of the row itself, and where the dword formulation finds the same halfword
                if (kb != 2 * h || p0 != 2 * h + 2 || p1 != 2 * h + 4) bad = 1;
                const uint32_t hw[3] = {h, h + 1, h + 2}, at[3] = {rh_row_lds_byte(kb, sw), rh_row_lds_byte(p0, sw), rh_row_lds_byte(p1, sw)};
                for (int q = 0; q < 3; ++q) {
                    const uint32_t d = hw[q] >> 1;
                    if (at[q] != (((((d >> 2) ^ sw) << 4) | ((d & 3) << 2)) + 2 * (hw[q] & 1))) bad = 1;
                }
                const uint32_t k2 = rd16(lds, at[0], &bad);
                const uint32_t pos2 = rd16(lds, at[1], &bad) | (rd16(lds, at[2], &bad) << 16);
                uint32_t key0, pos0; // and the row as the index build wrote it
                { uint16_t a; memcpy(&a, row + 8 + 6 * j, 2); key0 = a; memcpy(&pos0, row + 10 + 6 * j, 4); }
                if (bad || k2 != key || pos2 != pos || key != key0 || pos != pos0) {
                    printf("entry %u swizzle %u: key %x / %x / %x position %x / %x / %x%s\n", j, sw, k2, key, key0, pos2, pos, pos0, bad ? " (address)" : "");
                    fails++;
                }
            }
        }
    }
    // entries 6 and 14 are the ones whose position crosses a 16-byte piece
    for (uint32_t j = 0; j < 20; ++j) {
        const bool crosses = (rh_row_pos_byte(j, 0) >> 4) != (rh_row_pos_byte(j, 1) >> 4);
        if (crosses != (j == 6 || j == 14)) { printf("entry %u: crossing %d\n", j, (int)crosses); fails++; }
    }
    printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
"""


def _compile(src, exe, flags):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(ROOT, "real_amd", "csrc")] + flags +
                          [str(src), "-o", str(exe)], capture_output=True, text=True)


def test_row_bytes_equal_the_dword_formulation(tmp_path):
    src, exe = tmp_path / "row_bytes_check.cpp", tmp_path / "row_bytes_check"
    src.write_text(PROGRAM)
    r = _compile(src, exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(src, exe, [])     # a compiler without the sanitizer runtimes: the comparison itself still runs
    assert r.returncode == 0, r.stderr
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.strip().endswith("0 failures")


def test_header_is_hip_free():
    """(the host compiler builds it above; this pins what that relies on)"""
    text = open(os.path.join(ROOT, "real_amd", "csrc", "row_bytes.h")).read()
    assert "hip_runtime" not in text and "#include \"real_hip_internal.h\"" not in text
