"""Sweep of the rule the noise-mixing kernels inline (csrc/mix_rule.h) on the CPU: the stepped wrapped index against
``(s + t) % L`` for L in 1 .. 130, every s, strides 64 and 256; the chunk and lane decomposition and the tree against
the definition written out plainly, bit for bit, at n = 0, 1, 63, 64, 65, 16383, 16384, 16385, 32769, through arrays
exactly as long as the rule may touch; the plan's draws with ``x0 = x1 = 2^32 - 1``; the gain's zero cases with NaN; the
block counts with the refusal above 2^31 - 1 blocks; once more under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_mix_rule(tmp_path, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_mix_rule")
    src = os.path.join(ROOT, "tests", "csrc", "test_mix_rule.cpp")
    # (no contraction: every product and sum of the energy and the gain is rounded by itself, as in the kernels)
    subprocess.run([cxx, *flags, "-std=c++17", "-ffp-contract=off", src, "-o", exe, "-lm"], check=True,
                   capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "wrapped index: steps against the modulo" in res.stdout and "segment energy: chunks, lanes" in res.stdout
    assert "plan draws: Philox" in res.stdout and "gain: the zero cases" in res.stdout
    assert "block counts: the refusal" in res.stdout and "checks of the mix rule passed" in res.stdout
