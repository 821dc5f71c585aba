"""The host plan of node dict remode (csrc/node_remode_plan.hpp) on the CPU: the
join's window cuts for m in 0, 1, c - 1, c, c + 1 and a large m at one id per
window; storage capacities equal to ngpu_dict_retire's rule (and roomy enough for
an in-place extend of s / 2 rows); both scratch layouts aligned, without overlap
and exact; the split's verdict with the sum one short and one over; the slices'
verdict that bounds the join's copies; and the join's verdict over crafted
counters -- an id past the end, an id held twice, a missing position, the clean
case (tests/cpp/node_remode_plan_test.cpp, g++ with ASan/UBSan; no GPU)."""
import os
import subprocess

from conftest import ROOT


def test_node_remode_plan_cuts_caps_layouts_and_verdicts(tmp_path):
    exe = str(tmp_path / "node_remode_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nydus-snapshotter_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "node_remode_plan_test.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True, timeout=120)
    assert out.startswith("ok "), out
