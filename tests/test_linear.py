"""CPU tests of linear layers: the numpy checker tests/linear_checker.py against a big-integer Python loop
before the GPU tests compare words with it, the launch shapes of plan::plan_linear (cufhe_amd/csrc/launch_plan.h) through
tests/host/plan_linear_harness.cpp -- also built with the address and undefined-behaviour sanitizers and run as that program --, the
new symbols, and the refusals that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import linear_checker as lc
import oracle_lib as ol

NEW_SYMBOLS = ("cufhe_amd_linear_define", "cufhe_amd_linear_get", "cufhe_amd_linear_batch", "cufhe_amd_linear_list", "cufhe_amd_linear_gate_batch")
HARNESS_SRC = os.path.join(ol.ROOT, "tests", "host", "plan_linear_harness.cpp")
HARNESS = os.path.join(ol.ROOT, "tests", "host", "plan_linear_harness")
HARNESS_DEPS = [HARNESS_SRC, os.path.join(ol.ROOT, "cufhe_amd", "csrc", "launch_plan.h")]
WORDS = ol.LVL_WORDS                      # 631 and 1025: neither a multiple of 64


def test_library_exports_and_declares_the_new_entry_points():
    import cufhe_amd._lib as _lib
    import cufhe_amd.api as api
    lib = ctypes.CDLL(_lib.LIB_PATH)
    main = open(os.path.join(ol.ROOT, "include", "cufhe_amd.h")).read()
    part = open(os.path.join(ol.ROOT, "include", "cufhe_amd_linear.h")).read()
    assert '#include "cufhe_amd_linear.h"' in main, "include/cufhe_amd.h brings the declarations in"
    declared = re.sub(r"/\*.*?\*/", " ", part, flags=re.S)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.LINEAR_SIGNATURES, name
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, declared)
        assert proto, name
        assert len(proto.group(1).split(",")) == len(_lib.LINEAR_SIGNATURES[name][1]), name
    assert sorted(_lib.LINEAR_SIGNATURES) == sorted(set(re.findall(r"\b(cufhe_amd_[a-z0-9_]+)\s*\(", declared)))
    for name in ("define_linear", "linear_batch", "linear_list", "linear_gate_batch", "LinearLayer"):
        assert callable(getattr(api, name))
    shim = open(os.path.join(ol.ROOT, "include", "cufhe_amd.hpp")).read()
    for name in ("DefineLinear", "gLinear", "gLinearApply"):
        assert re.search(r"\b%s\s*\(" % name, shim), name


@pytest.mark.parametrize("rows,cols,sets,words", [(1, 1, 1, 1), (2, 3, 2, 3), (5, 4, 1, 2), (3, 7, 3, 5)])
def test_checker_is_the_defining_sum(rows, cols, sets, words):
    rng = np.random.default_rng(rows * 100 + cols)
    W = lc.test_weights(rng, rows, cols)
    x = lc.random_words(rng, sets, cols, words)
    x[0, 0, :] = 0xFFFFFFFF                                   # the largest word against the extreme weights
    bias = lc.random_words(rng, rows)
    for b in (bias, None):
        assert np.array_equal(lc.linear(W, b, x), lc.linear_bigint(W, b, x))


def test_checker_on_the_extreme_weights_alone():
    W = np.array([lc.EXTREME_WEIGHTS, lc.EXTREME_WEIGHTS[::-1]], np.int64)
    x = np.array([[[0xFFFFFFFF, 1], [0x80000000, 2], [0x7FFFFFFF, 3], [5, 0xFFFFFFFF]]], np.uint32)
    got = lc.linear(W, [1, 0xFFFFFFFF], x)
    assert np.array_equal(got, lc.linear_bigint(W, [1, 0xFFFFFFFF], x))
    # by hand, row 0 word 0: 2^31 (2^32 - 1) + (2^31 - 1) 2^31 - (2^31 - 1) + 0 = 2^31 + 2^31 + 2^31 + 1 mod 2^32 (no bias on word 0)
    assert int(got[0, 0, 0]) == (0x80000000 * 0xFFFFFFFF + 0x7FFFFFFF * 0x80000000 + 0xFFFFFFFF * 0x7FFFFFFF) % (1 << 32)
    # the bias lands on the last word only
    assert np.array_equal(lc.linear(W, [7, 9], x)[:, :, 0], lc.linear(W, None, x)[:, :, 0])
    assert np.array_equal(lc.linear(W, [7, 9], x)[0, :, 1], lc.linear(W, None, x)[0, :, 1] + np.array([7, 9], np.uint32))
    # a zero row gives the bias alone
    assert np.array_equal(lc.linear(np.zeros((1, 4), np.int64), [11], x)[0, 0], np.array([0, 11], np.uint32))


def _build(exe, flags):
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in HARNESS_DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, HARNESS_SRC])
    return exe


@pytest.fixture(scope="module")
def harness():
    return _build(HARNESS, [])


def plans(exe, requests):
    """[(rows, cols, sets, words, cus)] -> one dict per request"""
    out = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % r for r in requests), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-3000:]
    res = []
    for line in out.stdout.splitlines():
        f = line.split()
        assert f[0] == "plan"
        d = dict(zip(("rows", "cols", "sets", "words", "cus"), map(int, f[1:6])))
        d.update({f[i]: int(f[i + 1]) for i in (6, 8, 10, 12, 14, 16, 18, 20)})
        d["cover"] = (int(f[23]), int(f[24]))
        d["outside"] = int(f[26])
        res.append(d)
    assert len(res) == len(requests)
    return res


def sweep():
    """shapes around every boundary of the plan: the row tile, the 64-word chunk (words that are and are not multiples of it, both
    ciphertext sizes), one and several sets, devices small and large enough to flip the waves-per-workgroup rule"""
    TJ = 16
    reqs = []
    for rows in (1, TJ - 1, TJ, TJ + 1, 2 * TJ + 3, 4 * TJ, 4 * TJ + 1):
        for sets in (1, 3):
            for words in (1, 63, 64, 65, WORDS[0], WORDS[1]):
                for cus in (1, 40, 256):
                    reqs.append((rows, 67, sets, words, cus))
    reqs += [(1024, 1024, 4, WORDS[0], 256), (4096, 4096, 1, WORDS[0], 256), (64, 64, 64, WORDS[0], 256), (16384, 1, 1, WORDS[1], 304)]
    return reqs


def check_plans(res):
    for p in res:
        assert p["cover"] == (1, 1) and p["outside"] == 0, p
        TJ = p["row_tile"]
        assert p["row_tiles"] == -(-p["rows"] // TJ) and p["chunks"] == -(-p["words"] // 64)
        assert p["waves"] == p["sets"] * p["row_tiles"] * p["chunks"]
        # four waves per workgroup unless that leaves CUs without one
        assert p["per_block"] == (1 if -(-p["waves"] // 4) < p["cus"] else 4), p
        assert p["grid"] == -(-p["waves"] // p["per_block"]) and p["block"] == 64 * p["per_block"] <= 256


def test_plan_linear_covers_every_output_word_once(harness):
    res = plans(harness, sweep())
    check_plans(res)
    # the tile constants the GPU tests take their boundaries from are the plan's, and the kernel's
    assert {(p["row_tile"], p["unroll"]) for p in res} == {(lc_constant("kLinearRowTile"), lc_constant("kLinearUnroll"))}
    by = {(p["rows"], p["sets"], p["words"], p["cus"]): p for p in res}
    assert by[(4096, 1, WORDS[0], 256)]["grid"] == 640 and by[(1, 1, WORDS[0], 256)]["per_block"] == 1


def lc_constant(name):
    text = open(os.path.join(ol.ROOT, "cufhe_amd", "csrc", "launch_plan.h")).read()
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
    assert m, name
    return int(m.group(1))


def test_plan_linear_harness_under_the_sanitizers():
    """the same program built with -fsanitize=address,undefined, run stand-alone on the same sweep: no report, the same plans"""
    exe = _build(HARNESS + "_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    check_plans(plans(exe, sweep()))


def test_refusals_that_need_no_device_work():
    import cufhe_amd._lib as _lib
    lib = _lib.lib
    fake = ctypes.c_void_p(4096)                             # never dereferenced: every call is refused before any device work
    w = np.ones(4, np.int32)
    layer = ctypes.c_int(-1)

    def refused(rc, *words):
        msg = lib.cufhe_amd_last_error()
        assert rc == -1 and msg and all(x in msg for x in words), (rc, msg)

    refused(lib.cufhe_amd_linear_define(2, 2, None, None, ctypes.byref(layer)), b"null")
    refused(lib.cufhe_amd_linear_define(2, 2, w.ctypes.data, None, None), b"null")
    for rows, cols in ((0, 1), (1, 0), (16385, 1), (1, 16385), (16384, 8192)):
        refused(lib.cufhe_amd_linear_define(rows, cols, w.ctypes.data, None, ctypes.byref(layer)), b"16384")
    assert layer.value == -1
    # no layer is defined in this process: every id is unknown, the base id included
    for bad in (0, -1, 20480, 20480 + 63):
        refused(lib.cufhe_amd_linear_get(bad, None, None), b"not defined")
        refused(lib.cufhe_amd_linear_batch(0, None, bad, 0, 1, fake, 631, fake, 631), b"not defined")
        refused(lib.cufhe_amd_linear_list(0, None, bad, 0, 1, fake, fake), b"not defined")
        refused(lib.cufhe_amd_linear_gate_batch(0, None, bad, 1000, 0, 1, fake, 631, fake, 631), b"not defined")
    refused(lib.cufhe_amd_linear_batch(0, None, 20480, 0, 1, None, 631, fake, 631), b"null")
    refused(lib.cufhe_amd_linear_batch(0, None, 20480, 0, 1, fake, 631, None, 631), b"null")
    refused(lib.cufhe_amd_linear_list(0, None, 20480, 0, 1, None, fake), b"null")
    refused(lib.cufhe_amd_linear_list(0, None, 20480, 0, 1, fake, None), b"null")
    refused(lib.cufhe_amd_linear_gate_batch(0, None, 20480, 1000, 0, 1, fake, 631, None, 631), b"null")


def test_cpp_program_compiles():
    """tests/cpp/test_linear.cpp builds against include/cufhe_amd.hpp, the library and the oracle (it runs in the GPU suite)"""
    assert os.path.exists(lc.build_cpp_program())
