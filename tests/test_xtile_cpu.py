"""CPU-only: the x-column tile layout of a fused trajectory's k-space state and weights (barcode_amd/csrc/xtile.hpp),
compiled as plain C++ into a stand-alone program (tests/host/xtile_check.cpp) and run under AddressSanitizer /
UndefinedBehaviorSanitizer, built and run as tests/test_two_array_cpu.py does.  The program shows, for n = 32, 64, 128,
256, 512 in both precisions with the row strides the engine and the probe use, that

    xtile_index is a bijection on [0, Nhp), xtile_inverse inverts it and xtile_of is the same map of the linear index;
    every tile t = j (nhp / KB) + k0 / KB is one contiguous run of n KB elements, rows and lanes in order;
    a few elements worked out by hand land where they should;
    x_tiles is on for the benchmark's configuration at 128^3 and 256^3 and off for everything the issue lists,

and sweeps all 2^13 switch settings x the facts x 1 .. 4 steps for the invariant: wherever a boundary leaves a pair tiled,
the next kernel that reads that pair reads it tiled; a 3-D boundary on a tiled pair is refused; after the closing pass the
result is natural and nothing tiled is left."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_xtile_permutation_decision_and_layout_bookkeeping(tmp_path):
    exe = str(tmp_path / "xtile_check")
    # the sanitizer runtimes are linked statically, so the program does not care what else the process has preloaded
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", os.path.join(ROOT, "tests", "host", "xtile_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("xtile_check: ok"), r.stdout
    assert r.stderr == "", r.stderr
