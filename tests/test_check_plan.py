"""Check's bookkeeping (csrc/check_plan.hpp) on the CPU: the window planner --
every chunk in exactly one window, 16-byte aligned offsets, no window
overflows, a chunk exactly the size of the window is planned -- and the bitmap
decoder -- ascending ordinals, the cap honoured, the total equal to the
popcount (tests/cpp/check_plan_test.cpp, g++ with ASan/UBSan; no GPU)."""
import os
import subprocess

from conftest import ROOT


def test_check_window_planner_and_bitmap_decoder(tmp_path):
    exe = str(tmp_path / "check_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nydus-snapshotter_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "check_plan_test.cpp"), "-o", exe])
    for seed in ("1", "2", "3"):
        out = subprocess.check_output([exe, seed], text=True, timeout=120)
        assert out.startswith("ok 400"), out
