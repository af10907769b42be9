"""CPU-only: the image walker of barcode_amd/csrc/tile_walk.hpp (the index arithmetic of every tile kernel's fill and
flush), compiled as plain C++ into a stand-alone program (tests/host/tile_walk_check.cpp) and run under AddressSanitizer
/ UndefinedBehaviorSanitizer.  The program plays threads 0 .. 255 out in a loop on

    n = 16, 32, 48, 256 with 8 x 8 x 16 tiles and halo 2 (the 12 x 12 x 20 image; n = 16: the halo wraps onto the tile),
    n = 24 with 8 x 8 x 8 and n = 12 with 4 x 4 x 4 tiles, halo 2,
    n = 16, 32 with 8 x 8 x 16 tiles and halo 1 (the 10 x 10 x 18 image of the low-order kernels),
    n = 4 with its one 4 x 4 x 4 tile and halo 1, 2, 3 and 4 (halo 2: the image is (2 n)^3 and holds every cell 8 times),

every tile for n <= 48 and the 27 corner / edge-midpoint / face-centre / centre tiles of the lattice at n = 256, through
the run-time walker and, for the 12 x 12 x 20 image, through the compile-time instantiation of the 81-cell kernels as
well.  Every image cell must be visited exactly once and every (LDS index, global index) pair must equal the formula
the kernels used before (restated in the program).  An index error in the walker is an out-of-bounds access on the GPU:
this test is the proof that comes before any launch."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walker_visits_every_image_cell_once_with_the_old_indices(tmp_path):
    exe = str(tmp_path / "tile_walk_check")
    # the sanitizer runtimes are linked statically, so the program does not care what else the process has preloaded
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-static-libubsan", os.path.join(ROOT, "tests", "host", "tile_walk_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("tile_walk_check: ok"), r.stdout
    assert r.stderr == "", r.stderr
