"""Dict distill's host half (csrc/dict_distill_plan.hpp) on the CPU: the blob
remap from the live bitmap (no blob live, all live, the last dead, 2^20 blobs),
the blob id merge (the middle of three blobs of one id holds the only survivor; a
merge of blobs that all die), the KEEP_BLOBS identity, the scratch layout at m =
0, 1, 64, 65, 16,384 and 16,385, the histogram bucket edges and the info
(tests/cpp/dict_distill_plan_test.cpp, g++ with ASan/UBSan; no GPU)."""
import os
import subprocess

from conftest import ROOT


def test_dict_distill_plan_remap_merge_layout_and_info(tmp_path):
    exe = str(tmp_path / "dict_distill_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nydus-snapshotter_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "dict_distill_plan_test.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True, timeout=120)
    assert out.startswith("ok "), out
