"""Sweep of the rule the energy VAD kernels share (csrc/vad_rule.h) against brute force: the interleaved partial sums,
the threshold, the window, the vote and the decision kernel's walk over an utterance (CPU); once more under the address
and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_vad_rule(tmp_path, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_vad_rule")
    src = os.path.join(ROOT, "tests", "csrc", "test_vad_rule.cpp")
    subprocess.run([cxx, *flags, "-std=c++17", src, "-o", exe, "-lm"], check=True, capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "walks of the VAD rule checked" in res.stdout
