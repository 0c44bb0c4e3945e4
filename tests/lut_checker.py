"""Reference words of the encrypted-table lookup (cufhe_amd_lut_rotate_batch / _lut_lookup_batch / _trlwe_spread_batch, INTEGRATION.md
section 13), composed like tests/multi_output_checker.py: the roundings and SampleExtract(j) restated there, the CMux steps the
oracle's (orc_cmux), the key switch orc_keyswitch.  The one thing that differs from a user gate is the initial accumulator:
    acc_0 = (X^bbar A, X^bbar B)        for a table T = (A, B), a TRLWE of 2N words, instead of (0, X^bbar TV)
`spread` is the defining sum, term by term -- O(N reps), nothing shared with the kernel's prefix sums.  tests/test_lut.py shows that a
table (0, TV) reproduces multi_output_checker word for word and that pack + spread + lookup is a lookup, by decryption under genuine
keys, before the GPU tests compare words with this file."""
from concurrent.futures import ThreadPoolExecutor
import os
import subprocess

import numpy as np

import multi_output_checker as mc
import oracle_lib as ol
import user_gate_checker as uc

N, n, STEP_WORDS = uc.N, uc.n, uc.STEP_WORDS
M32 = 0xFFFFFFFF


def lut_rotate(keys, tlwe0, trlwe, s=0, steps=-1):
    """the accumulator (2N words) after `steps` CMux steps (outside [0, n]: all n) of the blind rotation of `tlwe0` from X^bbar trlwe"""
    tlwe0 = np.ascontiguousarray(tlwe0, np.uint32)
    trlwe = np.ascontiguousarray(trlwe, np.uint32).reshape(2 * N)
    if steps < 0 or steps > n:
        steps = n
    bbar = mc.ms_bbar(tlwe0[n], s)
    acc = np.concatenate([uc.negacyclic_rotate(trlwe[:N], bbar), uc.negacyclic_rotate(trlwe[N:], bbar)])
    res = np.empty(2 * N, np.uint32)
    for i in range(steps):
        abar = mc.ms_abar(tlwe0[i], s)
        rot = np.concatenate([uc.negacyclic_rotate(acc[:N], abar), uc.negacyclic_rotate(acc[N:], abar)])
        keys.L.orc_cmux(res, keys.bk[i * STEP_WORDS:(i + 1) * STEP_WORDS], rot, acc)
        acc, res = res, acc
    return acc


def lut_lookup(keys, tlwe0, trlwe, nout=1):
    """[nout][n + 1]: output j = KeySwitch(SampleExtract(j)(lut_rotate))"""
    acc = lut_rotate(keys, tlwe0, trlwe, mc.shift_of(nout))
    return np.stack([keys.keyswitch(mc.sample_extract(acc, j)) for j in range(nout)])


def on_threads(fn, count, threads=None):
    threads = threads or min(16, os.cpu_count() or 1)
    with ThreadPoolExecutor(threads) as ex:
        return list(ex.map(fn, range(count)))


def spread(trlwe, stride, reps):
    """X^(-stride (reps // 2)) sum_{i < reps} X^(i stride) c on both polynomials, mod 2^32, negacyclic: one term at a time"""
    assert stride >= 1 and reps >= 1 and stride * reps <= N
    c = np.ascontiguousarray(trlwe, np.uint32).reshape(2, N)
    out = np.zeros((2, N), np.uint64)
    for i in range(reps):
        e = (i * stride - stride * (reps // 2)) % (2 * N)
        for j in range(2):
            out[j] += uc.negacyclic_rotate(c[j], e)
    return (out & np.uint64(M32)).astype(np.uint32).reshape(2 * N)


def test_vector(values):
    """numpy restatement of cufhe_amd_test_vector: box m of N / p positions around m N / p holds values[m], the top half box -values[0]"""
    return mc.test_vector_multi(np.asarray(values, np.uint32)[None, :])


test_vector.__test__ = False


def build_cpp_program():
    """tests/cpp/test_lut.cpp -> tests/cpp/test_lut, with the flags tests/cpp_build.py gives the other C++ programs"""
    import cpp_build
    cdefs, libs = cpp_build.hip_flags()
    root = ol.ROOT
    exe = os.path.join(root, "tests", "cpp", "test_lut")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + cdefs +
                          ["-o", exe, os.path.join(root, "tests", "cpp", "test_lut.cpp"),
                           "-L" + os.path.join(root, "cufhe_amd"), "-lcufhe_amd", "-L" + os.path.join(root, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(root, "cufhe_amd"), "-Wl,-rpath," + os.path.join(root, "oracle")] + libs)
    return exe
