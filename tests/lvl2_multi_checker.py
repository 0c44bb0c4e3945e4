"""Reference words of the multi-output user gates of the N = 2048 ring (cufhe_amd_lvl2_define_gate_multi) and of the one-rotation
circuit bootstrap ("cb_rotations" 1), composed from tests/lvl2_user_gate_checker.py and tests/cb_checker.py.

What a multi-output rotation does differently from a single-output one is restated here in numpy (nbit = 11):
    abar_i = ((a_i + 2^(19+s)) >> (20+s)) << s,     bbar = 2 N2 - ((b >> (20+s)) << s)
    SampleExtract(j): out[m] = a[j - m] (m <= j), -a[N2 + j - m] (m > j), out[N2] = b[j]
The rotation itself is lvl2_user_gate_checker.blind_rotate_tv on a ciphertext whose words are the rounded ones put back at the bit
position the plain modulus switch reads (ms_rounded): the plain switch of that ciphertext IS the s-rounded switch of the original, so
every CMux step is the single-output checker's.  With s = 0 the ciphertext's switched words do not change at all
(tests/test_lvl2_multi_output_gates.py shows the equality with user_rotate_one and with cb_checker.blind_rotate_mu).  The key switch
is orc2_keyswitch.  Nothing here is shared with the kernels.  A rotation takes a second or two of CPU: callers compute references
once per module, on threads (on_threads).
"""
import numpy as np

import cb_checker as cb
import lvl2_user_gate_checker as lc
import oracle_lib as ol

n, N2 = ol.n, ol.N2
NBIT2 = cb.NBIT2
M64 = (1 << 64) - 1
LVL2_USER_OP_BASE, LVL2_MAX_USER_GATES = lc.LVL2_USER_OP_BASE, lc.LVL2_MAX_USER_GATES
LVL2_MAX_NOUT = 8
LVL2_USER_OP_LAST = LVL2_USER_OP_BASE + LVL2_MAX_NOUT * LVL2_MAX_USER_GATES - 1      # 8703
CB_SHIFT = 2
on_threads = lc.on_threads


def user_op_output(op, j):
    """CUFHE_AMD_LVL2_USER_OP_OUTPUT"""
    return op + j * LVL2_MAX_USER_GATES


def shift_of(nout):
    return {1: 0, 2: 1, 4: 2, 8: 3}[nout]


def ms_abar(a, s):
    return (((int(a) + (1 << (32 - 2 - NBIT2 + s))) & 0xFFFFFFFF) >> (32 - 1 - NBIT2 + s)) << s


def ms_bbar(b, s):
    return 2 * N2 - ((int(b) >> (32 - 1 - NBIT2 + s)) << s)


def ms_rounded(tlwe0, s):
    """the lvl0 ciphertext whose plain modulus switch (round a_i to 12 bits, truncate b) gives ms_abar(a_i, s) and ms_bbar(b, s)"""
    tlwe0 = np.ascontiguousarray(tlwe0, np.uint32)
    out = np.empty(n + 1, np.uint32)
    for i in range(n):
        out[i] = (ms_abar(tlwe0[i], s) << (32 - 1 - NBIT2)) & 0xFFFFFFFF
    out[n] = ((2 * N2 - ms_bbar(tlwe0[n], s)) << (32 - 1 - NBIT2)) & 0xFFFFFFFF
    return out


def blind_rotate_tv_multi(keys2, tlwe0, tv, s, steps=n):
    """the accumulator [2][N2] (uint64, flat) after `steps` steps from (0, X^bbar tv) with the modulus switch rounded to 2^s"""
    return lc.blind_rotate_tv(keys2, ms_rounded(tlwe0, s), tv, steps)


def sample_extract(acc, j):
    """SampleExtract(j) of the accumulator (a, b) of 2 N2 uint64 words: the lvl2 TLWE (N2 + 1 words) of coefficient j"""
    acc = np.ascontiguousarray(acc, np.uint64)
    a, b = acc[:N2], acc[N2:]
    m = np.arange(N2)
    out = np.empty(N2 + 1, np.uint64)
    lo = m <= j
    with np.errstate(over="ignore"):
        out[:N2][lo] = a[j - m[lo]]
        out[:N2][~lo] = np.uint64(0) - a[N2 + j - m[~lo]]
    out[N2] = b[j]
    return out


def multi_rotate_one(keys2, coeffs, off, tv, nout, ins, steps=n):
    """the one accumulator of an evaluation of a multi-output definition on single lvl0 ciphertexts ins"""
    x = lc.lincomb(coeffs, [np.ascontiguousarray(a, np.uint32) for a in ins[:lc.arity(coeffs)]], off)
    return blind_rotate_tv_multi(keys2, x, tv, shift_of(nout), steps)


def multi_extract_one(keys2, coeffs, off, tv, nout, ins):
    """[nout][N2 + 1]: every output of one evaluation before its key switch"""
    acc = multi_rotate_one(keys2, coeffs, off, tv, nout, ins)
    return np.stack([sample_extract(acc, j) for j in range(nout)])


def keyswitch(keys2, tlwe2):
    return keys2.keyswitch(tlwe2)


def test_vector_multi(values):
    """numpy restatement of cufhe_amd_lvl2_test_vector_multi: values [nout][p]; TV[nout q + j] = values[j][m], m the box of position
    nout q under lvl2_user_gate_checker.test_vector's boxes, the top half-box holds -values[j][0]"""
    values = np.asarray(values, np.uint64)
    nout, p = values.shape
    assert p >= 2 and p & (p - 1) == 0 and nout in (1, 2, 4, 8) and p * nout <= N2 // 2
    boxes = lc.test_vector(np.arange(p, dtype=np.uint64) + np.uint64(1))      # box index + 1; the top half-box reads 2^64 - 1
    tv = np.empty(N2, np.uint64)
    for q in range(N2 // nout):
        m = int(boxes[nout * q])
        for j in range(nout):
            tv[nout * q + j] = np.uint64((-int(values[j][0])) & M64) if m == M64 else values[j][m - 1]
    return tv


test_vector_multi.__test__ = False


def cb_test_vector():
    """the library's row: TVcb[4 q + r] = 2^(63 - 6 (r + 1)) for r < 3, TVcb[4 q + 3] = 0"""
    tv = np.zeros(N2, np.uint64)
    for r in range(cb.CB_L):
        tv[r::4] = np.uint64(cb.cb_mu(r))
    return tv


def cb_rotate_one(keys2, tlwe0):
    """stage 1 of one circuit bootstrap in the one-rotation form: [l][N2 + 1] uint64 -- SampleExtract(r) of ONE rotation with s = 2
    from TVcb, mu_r added to b"""
    acc = blind_rotate_tv_multi(keys2, tlwe0, cb_test_vector(), CB_SHIFT)
    out = np.zeros((cb.CB_L, cb.PKS_IN), np.uint64)
    with np.errstate(over="ignore"):
        for r in range(cb.CB_L):
            out[r] = sample_extract(acc, r)
            out[r, N2] += np.uint64(cb.cb_mu(r))
    return out


def cb_rotate_batch(keys2, tlwe0s):
    tlwe0s = np.ascontiguousarray(tlwe0s, np.uint32).reshape(-1, n + 1)
    return np.stack(on_threads(lambda g: cb_rotate_one(keys2, tlwe0s[g]), tlwe0s.shape[0]))
