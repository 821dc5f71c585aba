"""The host plan of retiring a partitioned node dict (csrc/node_retire_plan.hpp)
on the CPU: a part's scratch layout (aligned, no overlap, `bytes` exact) at m = 0,
1, 63, 64, 65 and the scan-tile edges for W = 1, 2, 8, 64; the capacities of the
parts' storages and of the node handle's rows; the verdict's refusals (each
counter, on each part; the parts' survivors not adding up to S; parts that
disagree about S; S > m) and what it accepts (a part with no survivor, S == 0,
S == m); and the global rank the compaction writes
(tests/cpp/node_retire_plan_test.cpp, g++ with ASan/UBSan; no GPU)."""
import os
import subprocess

from conftest import ROOT


def test_node_retire_plan_layout_verdict_and_capacities(tmp_path):
    exe = str(tmp_path / "node_retire_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nydus-snapshotter_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "node_retire_plan_test.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True, timeout=120)
    assert out.startswith("ok "), out
