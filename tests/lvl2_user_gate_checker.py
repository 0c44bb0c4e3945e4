"""Reference words of the user gates of the N = 2048 ring (cufhe_amd_lvl2_define_gate), composed from oracle pieces.

oracle/tfhe_oracle_lvl2.c hard-codes mu = 2^61 in its rotation, so the lvl02 rotation is restated here step by step from the pieces
of tests/cb_checker.py (_rotate64, _decomp_consts, the digit and orc2_polymul_ntt loop of blind_rotate_mu) with one change: the first
accumulator is (0, X^bar TV) for a caller's test vector of N2 uint64 words, bar = 2 N2 - (b >> 20), and bar = 2 N2 is the identity.
Around it: the lvl0 linear combination (numpy, mod 2^32), orc2_sample_extract0, orc2_keyswitch and the box builder of
cufhe_amd_lvl2_test_vector.  tests/test_lvl2_user_gates.py shows that this composition reproduces orc2_blind_rotate and orc2_gate word
for word before anything relies on it.  Nothing here is shared with the kernels.  A rotation takes a second or two of CPU: callers keep
word cases small and run them on threads (ctypes releases the GIL).
"""
from concurrent.futures import ThreadPoolExecutor
import os

import numpy as np

import cb_checker as cb
import oracle_lib as ol

n, N2 = ol.n, ol.N2
NBIT2 = cb.NBIT2
L2, BGBIT2, STEP2 = cb.L2, cb.BGBIT2, cb.STEP2
MU2 = ol.MU2
M64 = (1 << 64) - 1
LVL2_USER_OP_BASE, LVL2_MAX_USER_GATES = 8192, 64


def mu_test_vector():
    return np.full(N2, MU2, np.uint64)


def rotated_tv(tv, bar):
    """X^bar TV in Z_2^64[X]/(X^N2 + 1) for 1 <= bar <= 2 N2: coefficient e reads TV[(e - bar) mod N2], negated where
    (e < bar mod N2) xor (bar >= N2) -- except bar = 2 N2, the identity, which negates nothing"""
    tv = np.ascontiguousarray(tv, np.uint64)
    assert tv.shape == (N2,) and 1 <= bar <= 2 * N2
    if bar == 2 * N2:
        return tv.copy()
    with np.errstate(over="ignore"):
        return cb._rotate64(tv, bar)


def blind_rotate_tv(keys2, tlwe0, tv, steps=n):
    """the accumulator [2][N2] (uint64, flat) of the lvl02 rotation of lvl0 ciphertext tlwe0 starting from (0, X^bar tv)"""
    L = keys2.L
    tlwe0 = np.ascontiguousarray(tlwe0, np.uint32)
    if steps < 0 or steps > n:
        steps = n
    bar = 2 * N2 - cb._mod_switch(tlwe0[n])
    acc = np.zeros(2 * N2, np.uint64)
    acc[N2:] = rotated_tv(tv, bar)
    doff, roff = cb._decomp_consts()
    ro0 = 1 << (32 - 2 - NBIT2)
    res = np.zeros(N2, np.uint64)
    digits = np.zeros((2 * L2, N2), np.int32)
    with np.errstate(over="ignore"):
        for s in range(steps):
            abar = cb._mod_switch((int(tlwe0[s]) + ro0) & 0xFFFFFFFF)
            for j in range(2):
                t = cb._rotate64(acc[j * N2:(j + 1) * N2], abar) - acc[j * N2:(j + 1) * N2] + doff + roff
                for d in range(L2):
                    digits[j * L2 + d] = ((t >> np.uint64(64 - (d + 1) * BGBIT2)) & np.uint64((1 << BGBIT2) - 1)).astype(np.int64) - (1 << (BGBIT2 - 1))
            key = keys2.bk[s * STEP2:(s + 1) * STEP2]
            upd = np.zeros(2 * N2, np.uint64)
            for row in range(2 * L2):
                dr = np.ascontiguousarray(digits[row])
                for out in range(2):
                    L.orc2_polymul_ntt(res, dr, np.ascontiguousarray(key[(row * 2 + out) * N2:(row * 2 + out + 1) * N2]))
                    upd[out * N2:(out + 1) * N2] += res
            acc += upd
    return acc


def lincomb(coeffs, ins, off):
    """c0 in0 + c1 in1 + c2 in2 + (0, .., 0, off) mod 2^32 on lvl0 ciphertexts"""
    x = np.zeros(ins[0].shape, np.uint64)
    for c, a in zip(coeffs, ins):
        if c:
            x += (np.uint64(int(c) & 0xFFFFFFFF) * np.asarray(a).astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    x[..., -1] += np.uint64(int(off) & 0xFFFFFFFF)
    return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def arity(coeffs):
    c = list(coeffs) + [0] * (3 - len(coeffs))
    return 3 if c[2] else 2 if c[1] else 1


def user_rotate_one(keys2, coeffs, off, tv, ins, steps=n):
    x = lincomb(coeffs, [np.ascontiguousarray(a, np.uint32) for a in ins[:arity(coeffs)]], off)
    return blind_rotate_tv(keys2, x, tv if tv is not None else mu_test_vector(), steps)


def user_extract_one(keys2, coeffs, off, tv, ins):
    """the gate without its key switch: SampleExtract(0) of the full rotation, N2 + 1 uint64 words"""
    return keys2.sample_extract(user_rotate_one(keys2, coeffs, off, tv, ins))


def user_gate_one(keys2, coeffs, off, tv, ins):
    """one lvl2 user gate on single lvl0 ciphertexts ins: the words the library must return"""
    return keys2.keyswitch(user_extract_one(keys2, coeffs, off, tv, ins))


def on_threads(f, count, threads=None):
    threads = threads or min(16, os.cpu_count() or 1)
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(f, range(count)))


def test_vector(values):
    """cufhe_amd_lvl2_test_vector restated: coefficient j in [m N2/p - N2/(2p), m N2/p + N2/(2p)) holds values[m], the top half-box
    [N2 - N2/(2p), N2) holds -values[0]"""
    values = np.ascontiguousarray(values, np.uint64)
    p = values.size
    assert p >= 2 and p <= N2 // 2 and p & (p - 1) == 0
    box = N2 // p
    tv = np.empty(N2, np.uint64)
    for j in range(N2):
        lo = [m for m in range(p) if m * box - box // 2 <= j < m * box + box // 2]
        tv[j] = values[lo[0]] if lo else np.uint64((-int(values[0])) & M64)
    return tv


test_vector.__test__ = False


def signed64(x):
    """uint64 torus words as signed fractions of the torus"""
    return np.asarray(x, np.uint64).astype(np.int64).astype(np.float64) / 2.0 ** 64


def noise_sigmas():
    """INTEGRATION.md section 5.1, torus units, all derived from the parameters: (sigma of the lvl2 output, sigma of the lvl0 output,
    variance of the rotation, variance of the lvl20 key switch).
    rotation:   n steps of (k + 1) l N2 digits of variance Bg^2 / 12 against key noise alpha2 = 2^-44, plus the decomposition's
                rounding (Bg^-l / 2 = 2^-37 uniform) against 1 + N2 / 2 key bits;
    key switch: N2 t rows, 3 of 4 digits non-zero, of key noise alpha0 = 2^-15, plus the rounding to t basebit = 14 bits (2^-15
                uniform) against N2 / 2 key bits."""
    a0, a2 = 2.0 ** -15, 2.0 ** -44
    rotation = n * (2 * L2 * N2 * (2.0 ** BGBIT2) ** 2 / 12 * a2 ** 2 + (1 + N2 / 2) * (2.0 ** -37) ** 2 / 3)
    keyswitch = N2 * 7 * 0.75 * a0 ** 2 + (N2 / 2) * (2.0 ** -15) ** 2 / 3
    return np.sqrt(rotation), np.sqrt(rotation + keyswitch), rotation, keyswitch
