"""CPU test of the arithmetic behind keyswitch_mm_kernel (cufhe_amd/csrc/ks_matrix.h): tests/host/ks_matrix.cpp -- the balanced
base-256 split of the key words, the expansion of a 16-bit digit word into the 16 coefficients of an A fragment, the plane-wise
int32 product against the word-wise sum of keyswitch_kernel, and the bound of a plane sum -- compiled by plain g++ and run, once
as it is and once with the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ks_matrix.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_ks_matrix(build, tmp_path):
    exe = str(tmp_path / ("ks_matrix_" + build))
    subprocess.check_call(["g++", "-std=c++17"] + BUILDS[build] + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "0 checks failed" in out.stdout and "FAILED" not in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count(" ok\n") == 11
