"""The row cursor of the chunk-schedule SpMM kernels (gcn_amd/csrc/chunk_walk.h) built for the host with AddressSanitizer +
UndefinedBehaviorSanitizer and driven over seeded row pointers against a serial walk (tests/sanitize_chunk_walk.cpp): the
row-pointer arithmetic every one of those kernels runs, checked without a GPU."""
import os
import subprocess

from util import ROOT


def test_row_cursor_tiles_every_row_and_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sanitize_chunk_walk")
    build = subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-D_GLIBCXX_ASSERTIONS", "-Wall", "-Werror", os.path.join(ROOT, "tests", "sanitize_chunk_walk.cpp"),
                            "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    # 4 row counts x 2 chunk sizes x 8 matrices, each walked at 4 step sizes
    assert run.stdout.rstrip().endswith("chunk walk ok: 64 cases, 256 walks"), run.stdout[-500:]
