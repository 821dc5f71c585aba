"""Dict fold's host plan (csrc/dict_fold_plan.hpp) on the CPU: the blob-table
and placement decision tables, the layer-cut check, and the CPU restatement of
the kernels -- keep words, prefixes, every NEW chunk's record position and every
layer's blob rank -- against a brute-force walk over random kinds and layer cuts
at the sizes where a keep word, a workgroup and a scan tile end
(tests/cpp/dict_fold_plan_test.cpp, g++ with ASan/UBSan; no GPU)."""
import os
import subprocess

from conftest import ROOT


def test_dict_fold_plan_rules_positions_and_blob_ranks(tmp_path):
    exe = str(tmp_path / "dict_fold_plan_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nydus-snapshotter_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "dict_fold_plan_test.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True, timeout=120)
    assert out.startswith("ok "), out
