"""CPU-only: the two-array inverse side between the x and the y pass -- the launch shape of k_ypass_pair
(barcode_amd/csrc/pass_launch.hpp) and the decision which boundary kernels leave Psi^_x | B instead of the three Psi^
components (psi_pair, barcode_amd/csrc/eval_plan.hpp) --, compiled as plain C++ into a stand-alone program
(tests/host/two_array_check.cpp) and run under AddressSanitizer / UndefinedBehaviorSanitizer.  The program compares,
against literals worked out by hand,

    NT, PER, grid and LDS of k_ypass_pair at 128 / 256 / 512 in both precisions, and that no other n has a row;
    the decision at 256^3 and 512^3 (two arrays), and every case that keeps three: 128^3 without BCHMC_ZBIN_128, 64^3 and
    32^3, BCHMC_NO_PAIR, BCHMC_NO_PLANES, BCHMC_NO_ZBIN, calc_h 0 / 1 / 3, masskernel 0 / 1 / 2, the fallback sort, no
    tiles, the 3-D plans, ALPT,

and sweeps n = 16 .. 1024 x both precisions x all 2^10 switch settings x every configuration value x every fact x 1 .. 4
steps for the invariant that matters: wherever a boundary kernel leaves two arrays, the evaluation that reads them runs
the engine's own y pass, and that pass has a k_ypass_pair for this n."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_array_shapes_and_path_decision(tmp_path):
    exe = str(tmp_path / "two_array_check")
    # the sanitizer runtimes are linked statically, so the program does not care what else the process has preloaded
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", os.path.join(ROOT, "tests", "host", "two_array_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("two_array_check: ok"), r.stdout
    assert r.stderr == "", r.stderr
