"""CPU test of the tail of blind_rotate_kernel's CMux step: tests/host/root_products.cpp -- the products by the eighth roots of
unity, the last inverse pass built from them, the reduction schedule and the FP64 lift -- compiled by plain g++ and run, once as it
is and once with the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
SRC = os.path.join(HOST, "root_products.cpp")
DEPS = [SRC, os.path.join(HOST, "host_model.cpp")] + [os.path.join(ROOT, "cufhe_amd", "csrc", f) for f in ("fpfield.h", "ntt_r4.h", "ntt_tables.h")]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_root_products(build):
    exe = os.path.join(HOST, "root_products_" + build)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] + ["-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "0 checks failed" in out.stdout and "FAILED" not in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count(" ok\n") >= 13
