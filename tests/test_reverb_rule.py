"""Sweep of the rule the reverberation kernels inline (csrc/reverb_rule.h) on the CPU: the block, partition, pair and
output-range arithmetic against the definition written out plainly at n = 0, 1, 2, 511, 512, 513, 1023, 1024, 1025, 2049
and L = 1, 2, 511, 512, 513, 1024, 1025, 1537 (every d for the short L; 0, 1, 511, 512, L - 1 for the long ones): every
output sample written exactly once, no input index outside the utterance, the partitioned sum on integers equal to the
direct convolution, through arrays exactly as long as the rule may touch; the plan's draws with ``x0 = 2^32 - 1``; the
refusal above 2^31 - 1 blocks; once more under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_reverb_rule(tmp_path, flags):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "test_reverb_rule")
    src = os.path.join(ROOT, "tests", "csrc", "test_reverb_rule.cpp")
    subprocess.run([cxx, *flags, "-std=c++17", src, "-o", exe], check=True, capture_output=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "blocks, partitions, output ranges" in res.stdout and "plan draws: Philox" in res.stdout
    assert "launch counts: the refusal" in res.stdout and "checks of the reverb rule passed" in res.stdout
