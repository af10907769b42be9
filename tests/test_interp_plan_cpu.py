"""CPU-only: which kernel a bchmc_interp_particles call runs (barcode_amd/csrc/interp_plan.hpp: the tile kernel or the
direct one, the refusal of path = 1 where the tile kernel cannot run, the rule for path = -1), compiled as plain C++
into a stand-alone program (tests/host/interp_plan_check.cpp) and run under AddressSanitizer /
UndefinedBehaviorSanitizer against a table of cases."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_interp_path_decisions_give_the_values_worked_out_by_hand(tmp_path):
    exe = str(tmp_path / "interp_plan_check")
    # the sanitizer runtimes are linked statically, so the program does not care what else the process has preloaded
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", os.path.join(ROOT, "tests", "host", "interp_plan_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("interp_plan_check: ok"), r.stdout
    assert r.stderr == "", r.stderr


def test_the_header_has_no_hip_in_it():
    text = open(os.path.join(ROOT, "barcode_amd", "csrc", "interp_plan.hpp")).read()
    assert "#include <hip" not in text and "__device__" not in text and "__global__" not in text
