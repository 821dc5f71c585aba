"""Dict save's host plan (csrc/dict_save_plan.hpp) on the CPU: the file layout for
0, 1, 2^20 and 0xFFFFFFFE records with 0, 1, 15, 16, 17 and 2^20 blob rows (16 rows
fill 4096 bytes exactly, 17 pad to 8192), the header bytes, the window cuts for
window_records 1, 7, 64, k - 1, k and k + 1, and every refusal of the options
(tests/cpp/dict_save_plan_test.cpp, g++ with ASan/UBSan; no GPU)."""
import os
import subprocess

from conftest import ROOT


def test_dict_save_plan_layout_windows_and_refusals(tmp_path):
    exe = str(tmp_path / "dict_save_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nydus-snapshotter_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "dict_save_plan_test.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True, timeout=120)
    assert out.startswith("ok "), out
