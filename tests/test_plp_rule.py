"""Sweep of the rule the PLP kernel inlines (csrc/plp_rule.h) on the CPU: the row function against the definition
written out plainly, bit for bit, over F in {1, 2, 23, 40, 254}, p in {1, 2, 12, min(F + 1, 32)} and K in {1, p + 1},
through arrays exactly as long as the rule may touch; the known answers (an AR(1) spectrum, a flat one, the clamp, a
NaN row, a zero row); the lane and block mapping with the refusal above 2^31 - 1 blocks; once more under the address
and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_plp_rule(tmp_path, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_plp_rule")
    src = os.path.join(ROOT, "tests", "csrc", "test_plp_rule.cpp")
    # (no contraction: every product and sum of the recursions is rounded by itself, as in the kernel)
    subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", src, "-o", exe, "-lm"], check=True,
                   capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "rows against the definition written out" in res.stdout and "known answers" in res.stdout
    assert "lane and block mapping" in res.stdout and "checks of the PLP rule passed" in res.stdout
