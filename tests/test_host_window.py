"""The host pieces the windowed pipelines share (csrc/host_window.hpp) on the
CPU: each_set_bit against a bit-by-bit loop (range edges on and off word
boundaries, neighbours outside the range, a callback that stops, and
check_decode_bitmap on top of it against its earlier body), run_indexed (every
index once, no more than min(threads, items) threads, the caller among them),
read_exact (short reads continued; 0, an error or too much fail) and
host_threads (tests/cpp/host_window_test.cpp: g++ with ASan/UBSan, and once
more with TSan; no GPU)."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_host_window_pieces(tmp_path, sanitize):
    exe = str(tmp_path / "host_window_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=" + sanitize,
                           "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nydus-snapshotter_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "host_window_test.cpp"), "-o", exe,
                           "-lpthread"])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:exitcode=66")
    for seed in ("1", "2", "3"):
        r = subprocess.run([exe, seed], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stdout + r.stderr[-3000:]
        assert r.stdout.startswith("ok "), r.stdout
