"""The SHA-256 kernel selection rule (csrc/sha256_plan.hpp) on the CPU: the
pick of every admitted variant at n = 1, 31, 32, 33 and on both sides of the
auto thresholds 16384 and 32768, with `mixed` both ways; the launch shape of
every pick ((grid - 1) * chunks_per_wg < n <= grid * chunks_per_wg); and
sha_mixed at n % 32 of 0, 1 and 31 and one byte below, at and above the 15/16
threshold for the smallest and the largest chunk size
(tests/cpp/sha256_plan_test.cpp, g++ with ASan/UBSan; no GPU)."""
import subprocess

from sha_shapes import build_plan_test


def test_sha256_plan_picks_shapes_and_mixed_edges(tmp_path):
    exe = build_plan_test(str(tmp_path / "sha256_plan_test"))
    out = subprocess.check_output([exe], text=True, timeout=120)
    assert out.startswith("ok 128 picks"), out
