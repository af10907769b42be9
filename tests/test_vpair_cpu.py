"""CPU-only: the forward side with V as records and two arrays into the forward x pass -- the launch shape of
k_ypass_fwd_pair (barcode_amd/csrc/pass_launch.hpp) and the decisions v_pair / eval_vpair / v_rec
(barcode_amd/csrc/eval_plan.hpp) --, compiled as plain C++ into a stand-alone program (tests/host/vpair_check.cpp) and
run under AddressSanitizer / UndefinedBehaviorSanitizer.  The program compares, against literals worked out by hand,

    NT, PER, grid and LDS of k_ypass_fwd_pair at 128 / 256 / 512 in both precisions (ypair_grid, col_lds(.., 1)), and that
    no other n has a row;
    the predicates at 256^3 in both precisions, 128^3 with and without BCHMC_ZBIN_128, 512^3 (off: eval_yfwd keeps its
    values there), 32^3, ALPT, calc_h != 2, masskernel != 3, the general hull, BCHMC_NO_PLANES, BCHMC_NO_VPAIR, BCHMC_NO_VREC,

and sweeps n = 32 .. 1024 x both precisions x the 2^9 settings of the switches this side reads x the configuration
values x every fact x every evaluation mode for: never eval_vpair and eval_yfwd at once, eval_vpair => planes_r2c, v_rec => v_pair, v_pair => !alpt_x, v_pair => the y and z pass shapes
exist, and every evaluation of a fused trajectory that leaves two arrays is closed by a Zel'dovich k_step_boundary_x."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vpair_shapes_and_path_decision(tmp_path):
    exe = str(tmp_path / "vpair_check")
    # the sanitizer runtimes are linked statically, so the program does not care what else the process has preloaded
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", os.path.join(ROOT, "tests", "host", "vpair_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("vpair_check: ok"), r.stdout
    assert r.stderr == "", r.stderr
