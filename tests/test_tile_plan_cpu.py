"""CPU-only: the tile partition and the record-slot policy of barcode_amd/csrc/tile_plan.hpp (what a handle allocates for
the tile-sorted path, and when it re-partitions or reallocates the record array), compiled as plain C++ into a
stand-alone program (tests/host/tile_plan_check.cpp) and run under AddressSanitizer / UndefinedBehaviorSanitizer.  The
program compares, against literals worked out by hand,

    the hull for h = d and the partition at creation for n = 4, 5, 7, 9, 12, 24, 32, 128, 256, 1024, with the
    BCHMC_SORT_CAP / BCHMC_SORT_CAP_FIXED / BCHMC_CHUNK / BCHMC_NO_TILES / BCHMC_NO_TILES_LOW switches, mk = 1 with and
    without a grid origin, h = 0.86 d, and the memory budget for a small and a 288 GB device,
    the policy's answers to sequences of slot words: overflow, stale stamp, 3/4 and 7/8 thresholds, reallocation at a
    sync and deferred from inside a trajectory, the budget, the fall-back ladder, a pinned partition,

and sweeps the populations 1 .. 20000 for the invariants (whole segments, never shrinks, within the allocation, at most
2^30 - 8 slots per tile).  A mistake in this arithmetic is records written past the array on the GPU: this test is the
proof that comes before any launch."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_partition_and_slot_policy_give_the_values_worked_out_by_hand(tmp_path):
    exe = str(tmp_path / "tile_plan_check")
    # the sanitizer runtimes are linked statically, so the program does not care what else the process has preloaded
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", os.path.join(ROOT, "tests", "host", "tile_plan_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("tile_plan_check: ok"), r.stdout
    assert r.stderr == "", r.stderr
