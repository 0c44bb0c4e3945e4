"""Reference words of user gates on a compiled parameter set (cufhe_amd_ps_define_gate): tests/user_gate_checker.py made generic over
a loaded set oracle (ol.load_set(name)).

oracle/ hard-codes the constant mu in its blind rotation, so the rotation is rebuilt here step by step over the set's n, N, k:
    acc = (0, .., 0, X^bbar TV)                            numpy, negacyclic; k zero mask components
    acc <- orc_cmux(BK_i, X^abar_i acc, acc)   i < steps   = acc + BK_i [x] (X^abar_i acc - acc)
then SampleExtract at index j (numpy, k mask components) and orc_keyswitch.  A multi-output definition (shift s, 2^s outputs) rounds
abar_i and bbar to multiples of 2^s with the formulas of cufhe_amd/csrc/kernels_common.hip.h:78-80 on the set's Nbit.

`smallmod`: orc_evalkey_create switches the key to the P discretisation (orc_smallmod_from_torus) and orc_cmux does not, so the key
words handed to orc_cmux are mapped first -- vectorised here, pinned against the C function by tests/test_ps_user_gates.py, which also
shows that the whole composition reproduces orc_blind_rotate and orc_gate_batch on every set before anything relies on it.
"""
from concurrent.futures import ThreadPoolExecutor
import os
import subprocess

import numpy as np

import oracle_lib as ol

MU = ol.MU
SMALL_P = 625 * (1 << 20) + 1
M32 = np.uint64(0xFFFFFFFF)


def smallmod_from_torus(a):
    """round(a P / 2^32) of torus words, in [0, P]: orc_smallmod_from_torus, vectorised"""
    a = np.asarray(a, np.uint32).astype(np.uint64)
    return ((a * np.uint64(SMALL_P) + np.uint64(1 << 31)) >> np.uint64(32)).astype(np.uint32)


def negacyclic_rotate(p, e):
    """X^e p in Z[X]/(X^N + 1), N = len(p), any e >= 0 (X^2N = 1)"""
    N = p.size
    k = (np.arange(N, dtype=np.int64) - int(e)) % (2 * N)
    v = p[k % N]
    return np.where(k >= N, (0 - v.astype(np.uint64)).astype(np.uint32), v).astype(np.uint32)


def ms_abar(a, s, nbit):
    """kernels_common.hip.h:79 with the set's Nbit, 32-bit arithmetic"""
    return ((((int(a) + (1 << (32 - 2 - nbit + s))) & 0xFFFFFFFF) >> (32 - 1 - nbit + s)) << s)


def ms_bbar(b, s, nbit):
    """kernels_common.hip.h:80 with the set's Nbit"""
    return 2 * (1 << nbit) - ((int(b) >> (32 - 1 - nbit + s)) << s)


def lincomb(coeffs, ins, off):
    """c0 in0 + c1 in1 + c2 in2 + (0, .., 0, off) mod 2^32"""
    x = np.zeros(ins[0].shape, np.uint64)
    for c, a in zip(coeffs, ins):
        if c:
            x += (np.uint64(int(c) & 0xFFFFFFFF) * a.astype(np.uint64)) & M32
    x[..., -1] += np.uint64(int(off) & 0xFFFFFFFF)
    return (x & M32).astype(np.uint32)


def test_vector_multi(values, p, nout, N):
    """numpy restatement of cufhe_amd_ps_test_vector_multi: values [nout][p]; TV[nout q + j] = values[j][m], m = round(nout q p / N),
    the top half-box (m = p) -values[j][0]"""
    values = np.asarray(values, np.uint32).reshape(nout, p)
    box = N // p
    tv = np.empty(N, np.uint32)
    for q in range(N // nout):
        m = (nout * q + box // 2) // box
        for j in range(nout):
            tv[nout * q + j] = (0 - int(values[j][0])) & 0xFFFFFFFF if m == p else values[j][m]
    return tv


def test_vector(values, p, N):
    return test_vector_multi(values, p, 1, N)


test_vector.__test__ = test_vector_multi.__test__ = False       # helpers, not tests


class Checker:
    """the reference gate path of one parameter set"""

    def __init__(self, name, seed=5):
        self.name = name
        self.L = ol.load_set(name)
        self.K = ol.Keys(self.L, seed=seed)
        _, p = ol.set_params(self.L)
        self.n, self.N, self.k, self.nbit, self.l = p["n"], p["N"], p["k"], p["Nbit"], p["l"]
        self.words = self.K.words
        self.acc_words = (self.k + 1) * self.N
        self.step_words = (self.k + 1) * self.l * (self.k + 1) * self.N       # one TRGSW: (k+1) l rows of k+1 polynomials
        self.small = name == "smallmod"
        self.bk_cmux = smallmod_from_torus(self.K.bk) if self.small else self.K.bk

    def mu_test_vector(self):
        return np.full(self.N, MU, np.uint32)

    def rotate(self, tlwe0, tv=None, s=0, steps=-1):
        """the accumulator ((k+1) N words) after `steps` CMux steps (negative: all n) of the rotation of lvl0 ciphertext `tlwe0` that
        starts from (0, .., 0, X^bbar tv); tv None: mu everywhere"""
        N, k, n = self.N, self.k, self.n
        tlwe0 = np.ascontiguousarray(tlwe0, np.uint32)
        tv = self.mu_test_vector() if tv is None else np.ascontiguousarray(tv, np.uint32)
        acc = np.zeros(self.acc_words, np.uint32)
        acc[k * N:] = negacyclic_rotate(tv, ms_bbar(tlwe0[n], s, self.nbit))
        res = np.empty_like(acc)
        for i in range(n if steps < 0 or steps > n else steps):
            abar = ms_abar(tlwe0[i], s, self.nbit)
            rot = np.concatenate([negacyclic_rotate(acc[c * N:(c + 1) * N], abar) for c in range(k + 1)])
            self.L.orc_cmux(res, self.bk_cmux[i * self.step_words:(i + 1) * self.step_words], rot, acc)
            acc, res = res, acc
        return acc

    def sample_extract(self, acc, j=0):
        """SampleExtract at index j: per mask component c out[c N + m] = a_c[j - m] (m <= j), -a_c[N + j - m] (m > j); out[k N] = b[j]"""
        N, k = self.N, self.k
        out = np.empty(k * N + 1, np.uint32)
        m = np.arange(N)
        for c in range(k):
            a = acc[c * N:(c + 1) * N]
            out[c * N:(c + 1) * N] = np.where(m <= j, a[(j - m) % N], (0 - a[(N + j - m) % N].astype(np.uint64)).astype(np.uint32))
        out[k * N] = acc[k * N + j]
        return out

    def user_rotate_one(self, coeffs, off, tv, ins, s=0, steps=-1):
        """cufhe_amd_ps_user_rotate of one evaluation: lvl0 operands"""
        return self.rotate(lincomb(coeffs, [np.ascontiguousarray(a, np.uint32) for a in ins], off), tv, s, steps)

    def user_gate_one(self, level, coeffs, off, tv, ins, s=0):
        """one user gate on single ciphertexts of `level`: the [2^s][words] outputs the library must return"""
        x = lincomb(coeffs, [np.ascontiguousarray(a, np.uint32) for a in ins], off)
        if level == 0:
            acc = self.rotate(x, tv, s)
            return np.stack([self.K.keyswitch(self.sample_extract(acc, j)) for j in range(1 << s)])
        acc = self.rotate(self.K.keyswitch(x), tv, s)
        return np.stack([self.sample_extract(acc, j) for j in range(1 << s)])

    def encrypt_torus(self, level, msgs, sigma, seed):
        """TLWE encryptions of torus words `msgs` under the secret key of `level`, Gaussian noise of std `sigma` (torus words)"""
        rng = np.random.default_rng(seed)
        sk = self.K.key(level).astype(np.uint64)
        a = rng.integers(0, 1 << 32, size=(len(msgs), sk.size), dtype=np.uint64)
        e = np.rint(rng.normal(0.0, sigma, size=len(msgs))).astype(np.int64)
        b = ((a * sk).sum(axis=1) + np.asarray(msgs, np.uint64) + e.astype(np.uint64)) & M32
        return np.concatenate([a, b[:, None]], axis=1).astype(np.uint32)

    def phase(self, level, cts):
        """b - <a, s> mod 2^32 of each row"""
        cts = np.ascontiguousarray(cts, np.uint32).reshape(-1, self.words[level]).astype(np.uint64)
        sk = self.K.key(level).astype(np.uint64)
        return ((cts[:, -1] - (cts[:, :-1] * sk).sum(axis=1)) & M32).astype(np.uint32)


def on_threads(f, count, threads=None):
    """[f(0), .., f(count - 1)] on threads (ctypes releases the GIL in the oracle's calls)"""
    with ThreadPoolExecutor(threads or min(16, os.cpu_count() or 1)) as ex:
        return list(ex.map(f, range(count)))


def build_cpp_program():
    """tests/cpp/test_ps_user_gates.cpp -> tests/cpp/test_ps_user_gates over the `k2n512` set, with the flags tests/cpp_build.py gives
    the other C++ programs"""
    import cpp_build
    cdefs, libs = cpp_build.hip_flags()
    root = ol.ROOT
    ol.load_set("k2n512")
    exe = os.path.join(root, "tests", "cpp", "test_ps_user_gates")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DCUFHE_AMD_PARAM_SET_K2N512", "-DORC_SET_K2N512"] + cdefs +
                          ["-o", exe, os.path.join(root, "tests", "cpp", "test_ps_user_gates.cpp"),
                           "-L" + os.path.join(root, "cufhe_amd"), "-lcufhe_amd", "-L" + os.path.join(root, "oracle"), "-loracle_k2n512",
                           "-Wl,-rpath," + os.path.join(root, "cufhe_amd"), "-Wl,-rpath," + os.path.join(root, "oracle")] + libs)
    return exe
