"""Reference words of linear layers (cufhe_amd_linear_define / _linear_batch), in numpy.

    y[s][j][i] = ( sum_k (uint32)W[j][k] x[s][k][i]  +  (i == words - 1 ? bias[j] : 0) )  mod 2^32

The sum is evaluated in uint64: W is cast int32 -> int64 -> uint64 (sign extension, so the low 32 bits are (uint32)W), products and sums
wrap mod 2^64, and a wrap mod 2^64 preserves the value mod 2^32.  tests/test_linear.py holds this against a big-integer Python loop.
"""
import os
import subprocess

import numpy as np

import oracle_lib as ol

MASK = np.uint64(0xFFFFFFFF)
EXTREME_WEIGHTS = (-(1 << 31), (1 << 31) - 1, -1, 0)      # INT32_MIN, INT32_MAX, -1, 0


def linear(W, bias, x):
    """W [rows][cols] integers in int32 range; bias rows uint32 words or None; x [sets][cols][words] uint32 -> [sets][rows][words]"""
    W = np.asarray(W)
    assert W.ndim == 2 and W.min() >= -(1 << 31) and W.max() < (1 << 31)
    w64 = W.astype(np.int32).astype(np.int64).astype(np.uint64)
    x = np.ascontiguousarray(x, np.uint32)
    assert x.ndim == 3 and x.shape[1] == W.shape[1]
    # [rows][cols] @ [sets][cols][words]: uint64 matmul wraps mod 2^64
    y = np.einsum("jk,skw->sjw", w64, x.astype(np.uint64))
    if bias is not None:
        b = np.asarray(bias, np.uint64) & MASK
        assert b.shape == (W.shape[0],)
        y[:, :, -1] += b[None, :]
    return (y & MASK).astype(np.uint32)


def linear_bigint(W, bias, x):
    """the defining sum with Python integers, no wrap before the final reduction: for tiny shapes only"""
    W = [[int(v) for v in row] for row in np.asarray(W).tolist()]
    x = np.asarray(x)
    sets, cols, words = x.shape
    out = np.empty((sets, len(W), words), np.uint32)
    for s in range(sets):
        for j, row in enumerate(W):
            for i in range(words):
                acc = sum((row[k] % (1 << 32)) * int(x[s, k, i]) for k in range(cols))
                if bias is not None and i == words - 1:
                    acc += int(bias[j]) % (1 << 32)
                out[s, j, i] = acc % (1 << 32)
    return out


def test_weights(rng, rows, cols):
    """random int32 weights with the extreme values planted and one all-zero row (the last one, when there are at least two)"""
    W = rng.integers(-(1 << 31), 1 << 31, size=(rows, cols), dtype=np.int64)
    flat = W.reshape(-1)
    for n, v in enumerate(EXTREME_WEIGHTS):
        flat[(n * 7) % flat.size] = v
    if rows >= 2:
        W[rows - 1, :] = 0
    return W


test_weights.__test__ = False      # not a pytest test where it is imported by name


def random_words(rng, *shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


def build_cpp_program():
    """tests/cpp/test_linear.cpp -> tests/cpp/test_linear, with the flags tests/cpp_build.py gives the other C++ programs"""
    import cpp_build
    cdefs, libs = cpp_build.hip_flags()
    root = ol.ROOT
    exe = os.path.join(root, "tests", "cpp", "test_linear")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + cdefs +
                          ["-o", exe, os.path.join(root, "tests", "cpp", "test_linear.cpp"),
                           "-L" + os.path.join(root, "cufhe_amd"), "-lcufhe_amd", "-L" + os.path.join(root, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(root, "cufhe_amd"), "-Wl,-rpath," + os.path.join(root, "oracle")] + libs)
    return exe
