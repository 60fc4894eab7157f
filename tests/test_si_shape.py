"""Sweep of the short-integration kernels' launch-shape arithmetic (csrc/si_shape.h) against what the kernels rely on
(CPU); once more under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_si_shape(tmp_path, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_si_shape")
    src = os.path.join(ROOT, "tests", "csrc", "test_si_shape.cpp")
    subprocess.run([cxx, *flags, "-std=c++17", src, "-o", exe, "-lm"], check=True, capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "si shapes checked" in res.stdout
