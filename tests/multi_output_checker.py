"""Reference words of multi-output user gates (cufhe_amd_define_gate_multi), composed like tests/user_gate_checker.py.

The oracle has only orc_sample_extract0 and the modulus switch of the built-in gates, so the two things a multi-output gate does
differently are restated here in numpy:
    abar_i = ((a_i + 2^(30 - nbit + s)) >> (31 - nbit + s)) << s,   bbar = 2N - ((b >> (31 - nbit + s)) << s)
    SampleExtract(j): out[m] = a[j - m] (m <= j), -a[N + j - m] (m > j), out[N] = b[j]
The CMux steps are the oracle's (orc_cmux), the key switch is orc_keyswitch.  With s = 0 and j = 0 this is user_gate_checker word for
word (tests/test_multi_output_gates.py shows it), and the phase of SampleExtract(j) is coefficient j of the accumulator's phase.
"""
from concurrent.futures import ThreadPoolExecutor
import os

import numpy as np

import user_gate_checker as uc

N, n, NBIT, STEP_WORDS = uc.N, uc.n, uc.NBIT, uc.STEP_WORDS


def shift_of(nout):
    s = {1: 0, 2: 1, 4: 2, 8: 3}[nout]
    return s


def ms_abar(a, s):
    return (((int(a) + (1 << (30 - NBIT + s))) & 0xFFFFFFFF) >> (31 - NBIT + s)) << s


def ms_bbar(b, s):
    return 2 * N - ((int(b) >> (31 - NBIT + s)) << s)


def blind_rotate_tv_multi(keys, tlwe0, tv, s):
    """the accumulator (2N words) of a blind rotation of `tlwe0` from (0, X^bbar tv) with the modulus switch rounded to 2^s"""
    tlwe0 = np.ascontiguousarray(tlwe0, np.uint32)
    acc = np.zeros(2 * N, np.uint32)
    acc[N:] = uc.negacyclic_rotate(np.ascontiguousarray(tv, np.uint32), ms_bbar(tlwe0[n], s))
    res = np.empty(2 * N, np.uint32)
    for i in range(n):
        abar = ms_abar(tlwe0[i], s)
        rot = np.concatenate([uc.negacyclic_rotate(acc[:N], abar), uc.negacyclic_rotate(acc[N:], abar)])
        keys.L.orc_cmux(res, keys.bk[i * STEP_WORDS:(i + 1) * STEP_WORDS], rot, acc)
        acc, res = res, acc
    return acc


def sample_extract(acc, j):
    """SampleExtract(j) of a TRLWE (a, b) of 2N words: the lvl1 TLWE (N + 1 words) of coefficient j"""
    a, b = acc[:N].astype(np.uint32), acc[N:]
    m = np.arange(N)
    out = np.empty(N + 1, np.uint32)
    lo = m <= j
    out[:N][lo] = a[j - m[lo]]
    out[:N][~lo] = (0 - a[N + j - m[~lo]].astype(np.uint64)).astype(np.uint32)
    out[N] = b[j]
    return out


def multi_gate_one(keys, level, coeffs, off, tv, nout, ins, outputs=None):
    """all requested outputs (default: 0 .. nout - 1) of one evaluation on single ciphertexts ins: a list of words per output"""
    s = shift_of(nout)
    outputs = range(nout) if outputs is None else outputs
    x = uc.lincomb(coeffs, [np.ascontiguousarray(a, np.uint32) for a in ins], off)
    if level == 0:
        acc = blind_rotate_tv_multi(keys, x, tv, s)
        return [keys.keyswitch(sample_extract(acc, j)) for j in outputs]
    acc = blind_rotate_tv_multi(keys, keys.keyswitch(x), tv, s)
    return [sample_extract(acc, j) for j in outputs]


def multi_gate_batch(keys, level, coeffs, off, tv, nout, ins, threads=None):
    """multi_gate_one over rows: ins is a list of [count][words] arrays; returns [nout][count][words]"""
    count = ins[0].shape[0]
    threads = threads or min(16, os.cpu_count() or 1)
    with ThreadPoolExecutor(threads) as ex:
        rows = list(ex.map(lambda g: multi_gate_one(keys, level, coeffs, off, tv, nout, [a[g] for a in ins]), range(count)))
    return np.stack([np.stack([r[j] for r in rows]) for j in range(nout)])


def test_vector_multi(values):
    """numpy restatement of cufhe_amd_test_vector_multi: values [nout][p]"""
    values = np.asarray(values, np.uint32)
    nout, p = values.shape
    box = N // p
    tv = np.empty(N, np.uint32)
    for q in range(N // nout):
        m = (nout * q + box // 2) // box
        for j in range(nout):
            tv[nout * q + j] = (0 - int(values[j][0])) & 0xFFFFFFFF if m == p else values[j][m]
    return tv


def full_adder_tv(nout=2, p=4):
    """the one-bootstrap full adder of INTEGRATION.md: bits as padded p = 4 messages b / 8 (0 or mu = 2^29), x = a + b + cin; output 0
    = (x & 1) / 8, output 1 = (x >> 1) / 8 (further outputs, nout > 2, repeat them)"""
    mu = 1 << 29
    vals = [[(m & 1) * mu for m in range(p)], [((m >> 1) & 1) * mu for m in range(p)]]
    vals = (vals * (nout // 2 + 1))[:nout]
    return test_vector_multi(vals)


def decode(keys, level, cts, p=4):
    """messages m of padded p-ary encodings m 2^32 / (2p): the nearest m to each phase"""
    ph = uc.phase(keys, level, cts).astype(np.int64)
    return (np.rint(ph / float(1 << 32) * 2 * p).astype(np.int64)) % (2 * p)
