"""CPU-only: the launch shapes of the engine's own FFT passes (the arithmetic part of barcode_amd/csrc/pass_launch.hpp:
which instantiation, block size, dynamic LDS size and grid k_step_boundary_x / k_step_boundary_x2 / k_alpt_mix_x / k_ypass /
k_zr2c / k_zbin_direct get for a grid size and a precision), compiled as plain C++ into a stand-alone program
(tests/host/pass_launch_check.cpp) and run under AddressSanitizer / UndefinedBehaviorSanitizer.  The program compares,
against literals worked out by hand,

    KB, NT_BIG and NT_SMALL, every row of the x-pass, two-tile, y-pass and z-row tables, column and row LDS sizes, and the
    column (1 and 3 components, row stride from fft_host.hpp) and row grids, for fp64 and fp32,

and sweeps n = 1 .. 2048 for the invariants: PER * NT == n * KB, at most 1024 threads in whole waves, LDS within the
160 KiB of a CU, and "not available" for every n outside the tables (16, 48 and 1024 among them).  Both the engine and
the FFT-pass probes of tests/test_gpu_fft_passes.py launch through these tables."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass_shapes_give_the_values_worked_out_by_hand(tmp_path):
    exe = str(tmp_path / "pass_launch_check")
    # the sanitizer runtimes are linked statically, so the program does not care what else the process has preloaded
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", os.path.join(ROOT, "tests", "host", "pass_launch_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("pass_launch_check: ok"), r.stdout
    assert r.stderr == "", r.stderr
