"""CPU-only: which path a force evaluation takes (barcode_amd/csrc/eval_plan.hpp: planes mode or the 3-D plans, the fused
step boundary and its one-tile / two-tile / ALPT formulation, the ALPT pipeline on the 2-D plans, the z pass inside the
binning, the engine's own forward passes at 512^3), compiled as plain C++ into a stand-alone program
(tests/host/eval_plan_check.cpp) and run under AddressSanitizer / UndefinedBehaviorSanitizer.  The program compares,
against literals worked out by hand from the rules bchmc.hip held before the header existed,

    a 4-step trajectory at 256^3 step by step (fp64, fp32, BCHMC_BX_V1 / BX_V2, a field of 2^32 bytes), 512^3, 128^3,
    32^3 and 16^3, ALPT with and without its plans, a real-space mass, the GRF likelihood, BCHMC_NO_PLANES_ENDS, one
    step, and every refusal text of the fused z pass in the order the reasons are tested,

and sweeps n = 16 .. 1024 x both precisions x all 2^9 switch settings x every configuration value x every fact x
0 .. 4 steps for the invariants: no BX kernel without a row of the x-pass table, no two-tile kernel without its row or
with ALPT, no z pass inside the binning without planes_c2r and a z row, every step's evaluation finds in Ck what the
boundary before it left there, "runs" equals "reason is none"."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_path_decisions_give_the_values_worked_out_by_hand(tmp_path):
    exe = str(tmp_path / "eval_plan_check")
    # the sanitizer runtimes are linked statically, so the program does not care what else the process has preloaded
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", os.path.join(ROOT, "tests", "host", "eval_plan_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("eval_plan_check: ok"), r.stdout
    assert r.stderr == "", r.stderr
