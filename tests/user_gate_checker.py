"""Reference words of user gates (cufhe_amd_define_gate): the gate path with an arbitrary test vector, composed from oracle pieces.

oracle/ hard-codes the constant mu in its blind rotation, so the rotation is rebuilt here step by step:
    acc = (0, X^bbar TV)                                   numpy, negacyclic
    acc <- orc_cmux(BK_i, X^abar_i acc, acc)   i < n       = acc + BK_i [x] (X^abar_i acc - acc), the CMux of Accumulate
then orc_sample_extract0 and orc_keyswitch.  orc_bkgen's torus-domain key is [n][(k+1) l][k+1][N], so step i of it is exactly the
TRGSW orc_cmux takes; bbar and abar_i are computed with the roundings of orc_blind_rotate.  tests/test_user_gates.py shows that this
composition reproduces orc_gate word for word before anything relies on it.  It transforms the key again at every step: a
fraction of a second per rotation, so callers keep word-level cases small and run them on threads (ctypes releases the GIL).
"""
from concurrent.futures import ThreadPoolExecutor
import os
import subprocess

import numpy as np

import oracle_lib as ol

N, n = ol.N, ol.n
NBIT = 10
MU = ol.MU
STEP_WORDS = 2 * 3 * 2 * N          # one TRGSW: (k+1) l rows of k+1 polynomials


def mu_test_vector():
    return np.full(N, MU, np.uint32)


def negacyclic_rotate(p, e):
    """X^e p in Z[X]/(X^N + 1), 0 <= e <= 2N"""
    k = (np.arange(N, dtype=np.int64) - int(e)) % (2 * N)
    v = p[k % N]
    return np.where(k >= N, (0 - v.astype(np.uint64)).astype(np.uint32), v).astype(np.uint32)


def mod_switch(x):
    return int(x) >> (32 - 1 - NBIT)


def blind_rotate_tv(keys, tlwe0, tv):
    """the accumulator (2N words) of a blind rotation of lvl0 ciphertext `tlwe0` starting from (0, X^bbar tv)"""
    tlwe0 = np.ascontiguousarray(tlwe0, np.uint32)
    bbar = 2 * N - mod_switch(tlwe0[n])
    acc = np.zeros(2 * N, np.uint32)
    acc[N:] = negacyclic_rotate(np.ascontiguousarray(tv, np.uint32), bbar)
    roundoffset = 1 << (32 - 2 - NBIT)
    res = np.empty(2 * N, np.uint32)
    for i in range(n):
        abar = mod_switch((int(tlwe0[i]) + roundoffset) & 0xFFFFFFFF)
        rot = np.concatenate([negacyclic_rotate(acc[:N], abar), negacyclic_rotate(acc[N:], abar)])
        keys.L.orc_cmux(res, keys.bk[i * STEP_WORDS:(i + 1) * STEP_WORDS], rot, acc)
        acc, res = res, acc
    return acc


def lincomb(coeffs, ins, off):
    """c0 in0 + c1 in1 + c2 in2 + (0, .., 0, off) mod 2^32"""
    x = np.zeros(ins[0].shape, np.uint64)
    for c, a in zip(coeffs, ins):
        if c:
            x += (np.uint64(int(c) & 0xFFFFFFFF) * a.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    x[..., -1] += np.uint64(int(off) & 0xFFFFFFFF)
    return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def user_gate_one(keys, level, coeffs, off, tv, ins):
    """one user gate on single ciphertexts ins (1 to 3 arrays of the level's words): the words the library must return"""
    x = lincomb(coeffs, [np.ascontiguousarray(a, np.uint32) for a in ins], off)
    t1 = np.zeros(N + 1, np.uint32)
    if level == 0:
        acc = blind_rotate_tv(keys, x, tv)
        keys.L.orc_sample_extract0(t1, acc)
        return keys.keyswitch(t1)
    t0 = keys.keyswitch(x)
    acc = blind_rotate_tv(keys, t0, tv)
    keys.L.orc_sample_extract0(t1, acc)
    return t1


def user_gate_batch(keys, level, coeffs, off, tv, ins, threads=None):
    """user_gate_one over rows: ins is a list of [count][words] arrays; coeffs / off / tv per gate (lists) or shared"""
    count = ins[0].shape[0]
    per = lambda v: v if isinstance(v, list) else [v] * count  # noqa: E731
    cs, offs, tvs = per(coeffs), per(off), per(tv)
    threads = threads or min(16, os.cpu_count() or 1)
    with ThreadPoolExecutor(threads) as ex:
        rows = list(ex.map(lambda g: user_gate_one(keys, level, cs[g], offs[g], tvs[g] if tvs[g] is not None else mu_test_vector(),
                                                   [a[g] for a in ins]), range(count)))
    return np.stack(rows)


def encrypt_torus(keys, level, msgs, sigma, seed):
    """TLWE encryptions of torus words `msgs` under the oracle's secret key of `level`, Gaussian noise of std `sigma` (torus words)"""
    rng = np.random.default_rng(seed)
    s = keys.key(level).astype(np.uint64)
    dim = s.size
    a = rng.integers(0, 1 << 32, size=(len(msgs), dim), dtype=np.uint64)
    e = np.rint(rng.normal(0.0, sigma, size=len(msgs))).astype(np.int64)
    b = ((a * s).sum(axis=1) + np.asarray(msgs, np.uint64) + e.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    return np.concatenate([a, b[:, None]], axis=1).astype(np.uint32)


def phase(keys, level, cts):
    """b - <a, s> mod 2^32 of each row"""
    cts = np.ascontiguousarray(cts, np.uint32).reshape(-1, keys.words[level]).astype(np.uint64)
    s = keys.key(level).astype(np.uint64)
    return ((cts[:, -1] - (cts[:, :-1] * s).sum(axis=1)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def build_cpp_program():
    """tests/cpp/test_user_gates.cpp -> tests/cpp/test_user_gates, with the flags tests/cpp_build.py gives the other C++ programs"""
    import cpp_build
    cdefs, libs = cpp_build.hip_flags()
    root = ol.ROOT
    exe = os.path.join(root, "tests", "cpp", "test_user_gates")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + cdefs +
                          ["-o", exe, os.path.join(root, "tests", "cpp", "test_user_gates.cpp"),
                           "-L" + os.path.join(root, "cufhe_amd"), "-lcufhe_amd", "-L" + os.path.join(root, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(root, "cufhe_amd"), "-Wl,-rpath," + os.path.join(root, "oracle")] + libs)
    return exe
