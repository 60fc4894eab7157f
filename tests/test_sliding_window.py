"""Sweep of the window arithmetic the sliding-window CMVN kernels share (csrc/sliding_window.h) against its properties,
direct sums and the streaming ring walk (CPU); once more under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_sliding_window(tmp_path, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_sliding_window")
    src = os.path.join(ROOT, "tests", "csrc", "test_sliding_window.cpp")
    subprocess.run([cxx, *flags, "-std=c++17", src, "-o", exe, "-lm"], check=True, capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "sliding windows checked" in res.stdout
