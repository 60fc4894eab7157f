"""Sweep of the index arithmetic the rate-conversion kernels share (csrc/resample_index.h): output counts, phase and
base index against direct division (counts past 2^31 included) and the streaming due-count against a brute-force scan
(CPU); once more under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_resample_index(tmp_path, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_resample_index")
    src = os.path.join(ROOT, "tests", "csrc", "test_resample_index.cpp")
    subprocess.run([cxx, *flags, "-std=c++17", src, "-o", exe, "-lm"], check=True, capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "resample indices checked" in res.stdout
