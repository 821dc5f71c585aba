"""The host plan of distilling a partitioned node dict
(csrc/node_distill_plan.hpp) on the CPU: a part's scratch layout (aligned, no
overlap, `bytes` exact) at m_o and m = 0, 1, 63, 64, 65 and the scan-tile edges,
for W = 1, 2, 8, 64 and 0, 1, 32, 33 and 2^20 blobs; the info of the whole dict
(sums over the parts, the maximum of max_refs, the histogram adding up to
distinct); a part whose counters are not sane being refused; and the union of the
parts' live bitmaps through distill_blob_plan under each flag, with a blob live on
one part only (tests/cpp/node_distill_plan_test.cpp, g++ with ASan/UBSan; no GPU)."""
import os
import subprocess

from conftest import ROOT


def test_node_distill_plan_layout_sum_and_blob_union(tmp_path):
    exe = str(tmp_path / "node_distill_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nydus-snapshotter_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "node_distill_plan_test.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True, timeout=120)
    assert out.startswith("ok "), out
