"""Sweep of the rule the SpecAugment kernels share (csrc/specaug_rule.h) on the CPU: the three Philox known answers,
U's range, the plan's invariants for every T <= 300 and W <= 8 over many keys, the source position's monotonicity and
fixed points for every centre a plan may hold, a block's walk over its tile and a wave's partial sums lane by lane
through bounds-checked vectors against brute force, and the grid arithmetic at its refusal bounds; once more under the
address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_specaug_rule(tmp_path, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_specaug_rule")
    src = os.path.join(ROOT, "tests", "csrc", "test_specaug_rule.cpp")
    # (no contraction: the source position and the interpolation round every operation by itself, as the kernels do)
    subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", src, "-o", exe, "-lm"], check=True,
                   capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "tile walks and" in res.stdout and "checks of the SpecAugment rule passed" in res.stdout
