"""Dict retire's host plan (csrc/dict_retire_plan.hpp) on the CPU: the retire
bitmap and the blob remap at 1, 63, 64, 65 and 2^20 blobs (first, last, middle,
all, none, duplicates), the refusal of an index that equals the blob count, the
capacities of the result's storage, and that an extend of up to s / 2 rows after
a retire takes dict_grow_plan's share branch
(tests/cpp/dict_retire_plan_test.cpp, g++ with ASan/UBSan; no GPU)."""
import os
import subprocess

from conftest import ROOT


def test_dict_retire_plan_bitmap_remap_and_capacities(tmp_path):
    exe = str(tmp_path / "dict_retire_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nydus-snapshotter_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "dict_retire_plan_test.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True, timeout=120)
    assert out.startswith("ok "), out
