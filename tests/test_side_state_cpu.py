"""real_amd/csrc/side_table.h on the CPU: the table that keeps the stages' state beside the ctx (ctx_side.h) -- create on first
use, find without create, drop.

A stand-alone program (its own main, host compiler, address and undefined-behaviour sanitizers where the compiler has them)
over the header alone, with a payload that counts its constructions and destructions: a key's record is made once and stays
the same object; find makes nothing; drop destroys exactly that record and an unknown key's drop nothing; a key reused after a
drop gets a fresh record; two keys alive at once do not see each other's.  A second build under the thread sanitizer runs
eight threads on keys of their own through the one lock.  Nothing is loaded into Python.
"""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <atomic>
#include <stdio.h>
#include <thread>
#include <vector>
#include "side_table.h"

static std::atomic<int> made(0), gone(0);
struct Payload {
    int value = 7;          // what a fresh record reads
    long *heap;             // (owned: a record destroyed twice or never is the sanitizer's to report)
    Payload() : heap(new long(41)) { made++; }
    ~Payload() { delete heap; gone++; }
};
static RhSideTable<Payload> table;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s\n", __LINE__, #c); fails++; } } while (0)

int main(int argc, char **argv)
{
    int k1, k2; // two keys: their addresses
    if (argc > 1) {
        // eight threads, a key each: create, change, find, drop, again; no record is another thread's
        std::vector<std::thread> th;
        long keys[8];
        std::atomic<int> wrong(0);
        for (int t = 0; t < 8; ++t)
            th.emplace_back([&, t] {
                for (int r = 0; r < 200; ++r) {
                    Payload &p = table.at(&keys[t]);
                    if (p.value != 7) wrong++;
                    p.value = 100 + t;
                    Payload *q = table.find(&keys[t]);
                    if (q != &p || q->value != 100 + t) wrong++;
                    table.drop(&keys[t]);
                    if (table.find(&keys[t])) wrong++;
                }
            });
        for (auto &x : th) x.join();
        CHECK(wrong == 0);
        CHECK(made == 8 * 200 && gone == 8 * 200);
        printf("%d failures\n", fails);
        return fails ? 1 : 0;
    }
    // find without create
    CHECK(table.find(&k1) == nullptr && made == 0);
    table.drop(&k1); // (an unknown key: nothing)
    CHECK(made == 0 && gone == 0);
    // create on first use, once
    Payload &a = table.at(&k1);
    CHECK(made == 1 && a.value == 7 && *a.heap == 41);
    a.value = 1;
    CHECK(&table.at(&k1) == &a && table.find(&k1) == &a && made == 1);
    // two keys alive at once
    CHECK(table.find(&k2) == nullptr);
    Payload &b = table.at(&k2);
    b.value = 2;
    CHECK(made == 2 && &b != &a && table.at(&k1).value == 1 && table.at(&k2).value == 2);
    // drop: that record alone
    table.drop(&k1);
    CHECK(gone == 1 && table.find(&k1) == nullptr && table.find(&k2) == &b && b.value == 2);
    table.drop(&k1); // (twice: nothing)
    CHECK(gone == 1);
    // the key reused: a fresh record
    Payload &c = table.at(&k1);
    CHECK(made == 3 && c.value == 7 && table.find(&k2)->value == 2);
    table.drop(&k2);
    table.drop(&k1);
    CHECK(made == 3 && gone == 3 && !table.find(&k1) && !table.find(&k2));
    // what is still in the table at the end of the process stays (the map is never destroyed)
    table.at(&k2).value = 9;
    CHECK(made == 4 && gone == 3);
    printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
"""


def _compile(src, exe, flags):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    return subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", "-I", os.path.join(ROOT, "real_amd", "csrc")] + flags +
                          [str(src), "-o", str(exe)], capture_output=True, text=True)


def _run(exe, *args):
    p = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=120)
    print(p.stdout[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert p.stdout.strip().endswith("0 failures")


def test_create_find_drop_reuse_and_two_keys(tmp_path):
    src, exe = tmp_path / "side_table_check.cpp", tmp_path / "side_table_check"
    src.write_text(PROGRAM)
    r = _compile(src, exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _compile(src, exe, [])     # a compiler without the sanitizer runtimes: the checks themselves still run
    assert r.returncode == 0, r.stderr
    _run(exe)


def test_eight_threads_on_keys_of_their_own(tmp_path):
    src, exe = tmp_path / "side_table_check.cpp", tmp_path / "side_table_threads"
    src.write_text(PROGRAM)
    r = _compile(src, exe, ["-fsanitize=thread"])
    if r.returncode != 0:
        r = _compile(src, exe, [])     # a compiler without the thread sanitizer's runtime: the threads still run
    assert r.returncode == 0, r.stderr
    _run(exe, "threads")


def test_header_is_hip_free():
    """(the host compiler builds it above; this pins what that relies on)"""
    text = open(os.path.join(ROOT, "real_amd", "csrc", "side_table.h")).read()
    assert "hip_runtime" not in text and "#include \"real_hip_internal.h\"" not in text
