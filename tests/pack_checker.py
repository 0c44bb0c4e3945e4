"""Reference words of TLWE packing (cufhe_amd_pack_batch), straight from its formulas in numpy: integer
arithmetic mod 2^32, every comparison against these words is equality.

    abar_i = a_i + 2^15,  a_ij = (abar_i >> (32 - 2 (j + 1))) & 3                           j = 0 .. 7
    PackKS(x) = (0, b X^0) - sum_i sum_j [a_ij != 0] K[i][j][a_ij - 1]                      K: [n][t][3][2][N] uint32
    out[o] = sum over the inputs m with dst[m] = o of X^pos[m] PackKS(in[m])                X^e: negacyclic, both polynomials

Nothing here is shared with the kernel and the oracle has no counterpart, so tests/test_pack.py shows by decryption under a genuine
key (genuine_key below: K[i][j][v-1] = TRLWE_s1(v s0_i 2^(32 - 2 (j+1)))) that these formulas are a key switch."""
from concurrent.futures import ThreadPoolExecutor
import os
import subprocess

import numpy as np

import oracle_lib as ol

n, N = ol.n, ol.N
T, BASEBIT = 8, 2
NUMBASE = (1 << BASEBIT) - 1
ROW_WORDS = 2 * N
KEY_WORDS = n * T * NUMBASE * ROW_WORDS                  # 30 965 760
ROUND = 1 << (32 - T * BASEBIT - 1)                      # 2^15
KEY_SIGMA = 2.0 ** -25                                   # of the torus: the noise of a genuine key's rows
M32 = np.uint64(0xFFFFFFFF)
# input words at the edges of the digit decomposition: 0; both sides of the rounding boundary; where the carry of the rounding wraps
# to all-zero digits; all ones; a word whose 8 digits are all 3 (0xFFFF0000 + anything below 2^15)
EDGE_WORDS = (0x00000000, 0x00007FFF, 0x00008000, 0xFFFF7FFF, 0xFFFF8000, 0xFFFFFFFF, 0xFFFF0000, 0xFFFF7FFE)


def digits(x, rows=n):
    """[rows][t] digits 0 .. 3 of the first `rows` mask words of one lvl0 TLWE"""
    abar = (np.ascontiguousarray(x, np.uint32)[:rows].astype(np.uint64) + np.uint64(ROUND)) & M32
    sh = np.array([32 - BASEBIT * (j + 1) for j in range(T)], np.uint64)
    return ((abar[:, None] >> sh[None, :]) & np.uint64(NUMBASE)).astype(np.int64)


def pack_ks(key, x, rows=n):
    """PackKS(x), 2N words; `rows` < n: the sum over i < rows only (a key truncated in n: key is then [rows][t][3][2N])"""
    k = np.asarray(key).reshape(rows * T * NUMBASE, ROW_WORDS)
    a = digits(x, rows)
    ii, jj = np.nonzero(a)
    idx = (ii * T + jj) * NUMBASE + (a[ii, jj] - 1)
    s = k[idx].sum(axis=0, dtype=np.uint64)
    out = (np.uint64(0) - s) & M32
    out[N] = (out[N] + np.uint64(int(x[-1]))) & M32
    return out.astype(np.uint32)


def rotate(c, e):
    """X^e c on both polynomials, 0 <= e < N: coefficient k goes to k + e, negated past N"""
    c = np.ascontiguousarray(c, np.uint32).reshape(2, N)
    out = np.empty_like(c)
    neg = (np.uint64(0) - c.astype(np.uint64)) & M32
    out[:, e:] = c[:, :N - e]
    out[:, :e] = neg[:, N - e:].astype(np.uint32)
    return out.reshape(2 * N)


def pack_batch(key, ins, dst, pos, count_out, rows=n):
    """[count_out][2N] uint32"""
    ins = np.ascontiguousarray(ins, np.uint32).reshape(len(dst), -1)
    out = np.zeros((count_out, 2 * N), np.uint64)
    for m in range(len(dst)):
        out[int(dst[m])] += rotate(pack_ks(key, ins[m], rows), int(pos[m]))
    return (out & M32).astype(np.uint32)


def genuine_key(keys, seed, rows=n, threads=None):
    """K[i][j][v-1] = (a, a s1 + v s0_i 2^(32 - 2 (j+1)) X^0 + e) for i < rows: masks uniform, e Gaussian with sigma = 2^-25 of the torus,
    the products a s1 by orc_polymul_ntt (exact for a binary key) on threads"""
    L = keys.L
    rng = np.random.default_rng(seed)
    count = rows * T * NUMBASE
    key = np.empty((count, 2, N), np.uint32)
    key[:, 0] = rng.integers(0, 1 << 32, size=(count, N), dtype=np.uint64).astype(np.uint32)
    noise = np.rint(rng.normal(0.0, KEY_SIGMA * 2.0 ** 32, size=(count, N))).astype(np.int64)
    s1 = np.ascontiguousarray(keys.s1, np.uint32).astype(np.int32)

    def run(lo, hi):
        prod = np.zeros(N, np.uint32)
        for r in range(lo, hi):
            L.orc_polymul_ntt(prod, s1, key[r, 0])
            key[r, 1] = ((prod.astype(np.int64) + noise[r]) & 0xFFFFFFFF).astype(np.uint32)

    threads = threads or min(16, os.cpu_count() or 1)
    step = (count + threads - 1) // threads
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda t: run(t * step, min(count, (t + 1) * step)), range(threads)))
    r = np.arange(count)
    i, j, v = r // (T * NUMBASE), (r // NUMBASE) % T, r % NUMBASE + 1
    msg = (v.astype(np.uint64) * keys.s0[i].astype(np.uint64)) << (32 - BASEBIT * (j + 1)).astype(np.uint64)
    key[:, 1, 0] = ((key[:, 1, 0].astype(np.uint64) + msg) & M32).astype(np.uint32)
    return key.reshape(-1)


def trlwe_phase(keys, c):
    """b - a s1: the N phases of a TRLWE, the product by the oracle's schoolbook multiplication"""
    c = np.ascontiguousarray(c, np.uint32)
    prod = np.zeros(N, np.uint32)
    keys.L.orc_polymul_schoolbook(prod, np.ascontiguousarray(keys.s1, np.uint32).astype(np.int32), np.ascontiguousarray(c[:N]))
    return ((c[N:].astype(np.uint64) - prod.astype(np.uint64)) & M32).astype(np.uint32)


def tlwe0_phase(keys, x, rows=n):
    """b - sum_{i < rows} a_i s0_i of a lvl0 TLWE"""
    x = np.ascontiguousarray(x, np.uint32).astype(np.uint64)
    return (int(x[-1]) - int((x[:rows] * keys.s0[:rows].astype(np.uint64)).sum())) & 0xFFFFFFFF


def signed(d):
    """torus32 differences as signed integers in [-2^31, 2^31)"""
    return (np.asarray(d, np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)


def edge_inputs(rng, count):
    """[count][n + 1] random lvl0 words with the EDGE_WORDS sown in: input 0 is all edge words in turn, one input has every digit 3,
    the others carry an edge word every 7th position"""
    x = rng.integers(0, 1 << 32, size=(count, n + 1), dtype=np.uint64).astype(np.uint32)
    e = np.array(EDGE_WORDS, np.uint32)
    x[0, :n] = e[np.arange(n) % len(e)]
    if count > 1:
        x[1, :n] = np.uint32(0xFFFF0000) + rng.integers(0, 1 << 15, size=n, dtype=np.uint64).astype(np.uint32)
    for m in range(2, count):
        x[m, m % 7:n:7] = e[(np.arange(len(x[m, m % 7:n:7])) + m) % len(e)]
    return x


def build_cpp_program():
    """tests/cpp/test_pack.cpp -> tests/cpp/test_pack, with the flags tests/cpp_build.py gives the other C++ programs"""
    import cpp_build
    cdefs, libs = cpp_build.hip_flags()
    root = ol.ROOT
    exe = os.path.join(root, "tests", "cpp", "test_pack")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + cdefs +
                          ["-o", exe, os.path.join(root, "tests", "cpp", "test_pack.cpp"),
                           "-L" + os.path.join(root, "cufhe_amd"), "-lcufhe_amd", "-L" + os.path.join(root, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(root, "cufhe_amd"), "-Wl,-rpath," + os.path.join(root, "oracle")] + libs)
    return exe
