"""CPU-only: the resource owners of barcode_amd/csrc/owned.hpp, compiled into a stand-alone program against a stand-in
runtime (tests/host/owned_check.cpp) and run under AddressSanitizer / UndefinedBehaviorSanitizer.  The program checks
the live counts after every step; the sanitizers, LeakSanitizer included, must have nothing to say."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_owners_under_address_sanitizer(tmp_path):
    exe = str(tmp_path / "owned_check")
    # g++ and no HIP runtime library: every runtime function owned.hpp calls is defined by the program itself.  The
    # sanitizer runtimes are linked statically, so the program does not care what else the process has preloaded.
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-pthread", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(ROCM, "include"), "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           os.path.join(ROOT, "tests", "host", "owned_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "owned_check: ok"
    assert r.stderr == "", r.stderr
