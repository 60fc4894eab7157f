"""Sweep of the rule the PCEN kernels share (csrc/pcen_rule.h) against brute force: the lane -> (utterance, column)
mapping and the lane and block counts around 255 / 256 / 257 lanes and past 2^32, the refusal above 2^31 - 1 blocks,
the smoother step and a lane's walk over an utterance (CPU); once more under the address and undefined-behaviour
sanitizers."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_pcen_rule(tmp_path, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_pcen_rule")
    src = os.path.join(ROOT, "tests", "csrc", "test_pcen_rule.cpp")
    # (no contraction: the smoother's two products and its sum are each rounded once, as the kernels are built)
    subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", src, "-o", exe, "-lm"], check=True,
                   capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "walks of the PCEN smoother checked" in res.stdout and "checks of the PCEN rule passed" in res.stdout
