"""Reference words of the packed-ROM operations, composed from oracle pieces the suite already trusts.
Everything is integer arithmetic mod 2^32: every comparison against these words is equality, no tolerance.

    rotation              negacyclic_rotate (tests/user_gate_checker.py) on both polynomials of a TRLWE
    rotating CMUX         orc_cmux(res, trgsw, rotate(c, e), c) with the torus-domain TRGSW whose NTT image the GPU gets
    extraction at j, (1)  numpy from out[m] = a[j - m] (m <= j), -a[N + j - m] (m > j), out[N] = b[j]
    extraction at j, (2)  orc_sample_extract0 of rotate(c, 2N - j): SE_j(c) = SE_0(X^-j c); j = 0: orc_sample_extract0(c)
    key switch            Keys.keyswitch
tests/test_packed_rom.py shows that (1) and (2) agree before anything relies on either.
"""
import os
import subprocess

import numpy as np

import oracle_lib as ol
from user_gate_checker import negacyclic_rotate, STEP_WORDS

N, n = ol.N, ol.n
MU = ol.MU
EXPONENTS = (0, 1, 63, 64, 1023, 1024, 1025, 2047)       # both sides of the wave's rows (64), of the wrap (N) and the ends
INDICES = (0, 1, 2, 63, 64, 511, 1022, 1023)
TL_SEIKS_AT_BASE, TL_CMUX_ROTATE_BASE = 2048, 4096        # include/cufhe_amd.h


def rotate(c, e):
    """X^e c on both polynomials of a TRLWE (2N words), 0 <= e < 2N"""
    c = np.ascontiguousarray(c, np.uint32)
    return np.concatenate([negacyclic_rotate(c[:N], e), negacyclic_rotate(c[N:], e)])


def cmux(L, trgsw, c1, c0):
    res = np.zeros(2 * N, np.uint32)
    L.orc_cmux(res, np.ascontiguousarray(trgsw, np.uint32).ravel(), np.ascontiguousarray(c1, np.uint32), np.ascontiguousarray(c0, np.uint32))
    return res


def cmux_rotate(L, trgsw, c, e):
    """c + trgsw [x] (X^e c - c)"""
    return cmux(L, trgsw, rotate(c, e), c)


def extract_formula(c, j):
    """SampleExtract(j), option 1: the formula, in numpy"""
    c = np.ascontiguousarray(c, np.uint32)
    a, b = c[:N], c[N:]
    m = np.arange(N)
    low = a[(j - m) % N]
    out = np.where(m <= j, low, (0 - a[(N + j - m) % N].astype(np.uint64)).astype(np.uint32)).astype(np.uint32)
    return np.concatenate([out, b[j:j + 1]]).astype(np.uint32)


def extract_by_rotation(L, c, j):
    """SampleExtract(j), option 2: the oracle's extraction at 0 of X^-j c"""
    t1 = np.zeros(N + 1, np.uint32)
    L.orc_sample_extract0(t1, np.ascontiguousarray(c, np.uint32) if j == 0 else rotate(c, 2 * N - j))
    return t1


def extract_keyswitch(keys, c, j):
    return keys.keyswitch(extract_by_rotation(keys.L, c, j))


def encrypt_trlwe(keys, msgs, sigma, seed):
    """a TRLWE encryption (2N words) of the torus polynomial `msgs` under the oracle's lvl1 key: b = a s + msgs + e"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
    e = np.rint(rng.normal(0.0, sigma, size=N)).astype(np.int64).astype(np.uint64)
    prod = np.zeros(N, np.uint32)
    keys.L.orc_polymul_schoolbook(prod, np.ascontiguousarray(keys.s1, np.uint32).astype(np.int32), a)
    b = (prod.astype(np.uint64) + np.asarray(msgs, np.uint32).astype(np.uint64) + e) & np.uint64(0xFFFFFFFF)
    return np.concatenate([a, b.astype(np.uint32)])


def trlwe_phase(keys, c):
    """b - a s: the N phases of a TRLWE"""
    c = np.ascontiguousarray(c, np.uint32)
    prod = np.zeros(N, np.uint32)
    keys.L.orc_polymul_schoolbook(prod, np.ascontiguousarray(keys.s1, np.uint32).astype(np.int32), np.ascontiguousarray(c[:N]))
    return ((c[N:].astype(np.uint64) - prod.astype(np.uint64)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def selector(keys, bit, which=0):
    """a torus-domain TRGSW encryption of `bit` under the lvl1 key: step i of the oracle's bootstrapping key is TRGSW(s0[i]), so the
    `which`-th step whose key bit is `bit` is a valid selector of that bit made by the oracle's own generator"""
    i = int(np.flatnonzero(keys.s0 == bit)[which])
    return np.ascontiguousarray(keys.bk[i * STEP_WORDS:(i + 1) * STEP_WORDS])


# The recorded program of the tests: 2 TRLWEs of 4 words of 8 bits, bit b of word w at coefficient 8 w + b, messages +-mu; address
# bits a0, a1 bring word (a0 + 2 a1) of both TRLWEs to the front, a2 picks the TRLWE, the 8 bits come out at indices 0 .. 7.
ROM_WORD_BITS, ROM_WORDS_PER_TRLWE, ROM_TRLWES = 8, 4, 2
ROM_EXPONENTS = (2 * N - 8, 2 * N - 16)


def rom_table(seed):
    """[2][4] words of 8 bits"""
    return np.random.default_rng(seed).integers(0, 256, size=(ROM_TRLWES, ROM_WORDS_PER_TRLWE)).astype(np.uint32)


def rom_trlwes(keys, table, seed, sigma=64.0):
    out = []
    for t in range(ROM_TRLWES):
        msgs = np.zeros(N, np.uint32)        # coefficients past the words hold 0: never read
        for w in range(ROM_WORDS_PER_TRLWE):
            for b in range(ROM_WORD_BITS):
                msgs[ROM_WORD_BITS * w + b] = MU if (int(table[t, w]) >> b) & 1 else (1 << 32) - MU
        out.append(encrypt_trlwe(keys, msgs, sigma, seed + t))
    return out


def rom_read(keys, trlwes, selectors):
    """the oracle composition of the recorded program: 8 lvl0 ciphertexts [8][n + 1]"""
    L = keys.L
    c = [np.array(t, np.uint32) for t in trlwes]
    for t in range(ROM_TRLWES):
        for k, e in enumerate(ROM_EXPONENTS):
            c[t] = cmux_rotate(L, selectors[k], c[t], e)
    r = cmux(L, selectors[2], c[1], c[0])
    return np.stack([extract_keyswitch(keys, r, b) for b in range(ROM_WORD_BITS)])


def build_cpp_program():
    """tests/cpp/test_packed_rom.cpp -> tests/cpp/test_packed_rom, with the flags tests/cpp_build.py gives the other C++ programs"""
    import cpp_build
    cdefs, libs = cpp_build.hip_flags()
    root = ol.ROOT
    exe = os.path.join(root, "tests", "cpp", "test_packed_rom")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + cdefs +
                          ["-o", exe, os.path.join(root, "tests", "cpp", "test_packed_rom.cpp"),
                           "-L" + os.path.join(root, "cufhe_amd"), "-lcufhe_amd", "-L" + os.path.join(root, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(root, "cufhe_amd"), "-Wl,-rpath," + os.path.join(root, "oracle")] + libs)
    return exe
