"""fmx_common.hpp mdiv_rank (the fused pass's rank output: an integer numerator, so mdiv's
range guard is a test of the integer) returns the IEEE quotient bit for bit and takes the IEEE
divide exactly where mdiv's exponent guard did: 1.1e8 host cases (tests/native/mdiv_rank_check.c),
every numerator of every row length up to 8200 and of the 100 longest, the guard boundary
(numerator 0, 1) included.  The GPU side is pinned by tests/test_gpu_fused_diet.py."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_mdiv_rank_matches_ieee_division(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no host C compiler")
    exe = tmp_path / "mdiv_rank_check"
    c = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", str(exe),
                        os.path.join(HERE, "native", "mdiv_rank_check.c"), "-lm"], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr                 # a check file that does not compile fails
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr + p.stdout
    assert "0 mismatches" in p.stdout
