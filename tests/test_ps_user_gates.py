"""User gates on the compiled parameter sets (cufhe_amd_ps_define_gate), the parts that need no GPU: the C surface and its id range,
the host-only test-vector builders against a numpy restatement, and tests/ps_user_gate_checker.py -- the reference every GPU
comparison of tests/test_gpu_ps_user_gates.py relies on -- against the set oracles it is composed from."""
import ctypes
import os
import re

import numpy as np
import pytest

import footprint as fp
import oracle_lib as ol
import ps_user_gate_checker as pc

ROOT = ol.ROOT
LIB = os.path.join(ROOT, "cufhe_amd", "libcufhe_amd.so")
NEW = ("cufhe_amd_ps_define_gate", "cufhe_amd_ps_define_gate_multi", "cufhe_amd_ps_test_vector", "cufhe_amd_ps_test_vector_multi",
       "cufhe_amd_ps_user_rotate")
NAND = ol.OPS.index("NAND")


@pytest.fixture(scope="module")
def lib():
    return ctypes.CDLL(LIB)


def _header():
    return open(os.path.join(ROOT, "include", "cufhe_amd.h")).read()


def _define(text, name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % re.escape(name), text).group(1))


# ---- symbols and ids ----
def test_new_symbols_are_exported_and_bound(lib):
    from cufhe_amd import _lib
    for s in NEW:
        assert hasattr(lib, s), f"{s} is not exported"
        assert s in _lib.SIGNATURES, f"{s} is not in _lib.SIGNATURES"
    # none of them is a `_batch` entry point: the footprint table of tests/footprint.py is the parent's, every symbol has its case
    symbols = fp.header_batch_symbols()
    assert not set(NEW) & set(symbols)
    assert sorted(symbols) == sorted(fp.CASES)


def test_id_range_overlaps_no_other_range():
    h = _header()
    base, cap = _define(h, "CUFHE_AMD_PS_USER_OP_BASE"), _define(h, "CUFHE_AMD_PS_MAX_USER_GATES")
    assert (base, cap) == (12288, 64)
    mine = range(base, base + 8 * cap)                       # output j of definition k: base + k + 64 j, j < 8
    n1024 = 1024
    others = {
        "built-in and TRLWE-level ops": range(0, 1000),
        "user gates": range(_define(h, "CUFHE_AMD_USER_OP_BASE"), _define(h, "CUFHE_AMD_USER_OP_BASE") + 8 * _define(h, "CUFHE_AMD_MAX_USER_GATES")),
        "SEIKS_AT": range(_define(h, "CUFHE_AMD_TL_SEIKS_AT_BASE"), _define(h, "CUFHE_AMD_TL_SEIKS_AT_BASE") + n1024),
        "CMUX_ROTATE": range(_define(h, "CUFHE_AMD_TL_CMUX_ROTATE_BASE"), _define(h, "CUFHE_AMD_TL_CMUX_ROTATE_BASE") + 2 * n1024),
        "lvl2 user gates": range(_define(h, "CUFHE_AMD_LVL2_USER_OP_BASE"),
                                 _define(h, "CUFHE_AMD_LVL2_USER_OP_BASE") + 8 * _define(h, "CUFHE_AMD_LVL2_MAX_USER_GATES")),
    }
    for name, r in others.items():
        assert r.stop <= mine.start or mine.stop <= r.start, f"the parameter sets' user op ids overlap the {name}"
    from cufhe_amd import api
    assert (api.PS_USER_OP_BASE, api.PS_MAX_USER_GATES) == (base, cap)
    assert api.ps_user_op_output(base + 5, 3) == base + 5 + 3 * cap


# ---- the test-vector builders (host only) ----
def _set_index(lib, name):
    from cufhe_amd import _lib
    p = _lib.PsParams()
    lib.cufhe_amd_ps_get_params.argtypes = [ctypes.c_int, ctypes.POINTER(_lib.PsParams)]
    for i in range(lib.cufhe_amd_ps_count()):
        assert lib.cufhe_amd_ps_get_params(i, ctypes.byref(p)) == 0
        if p.name.decode() == name:
            return i, int(p.N)
    raise KeyError(name)


def _c_test_vector(lib, idx, N, values, p, nout):
    values = np.ascontiguousarray(values, np.uint32)
    tv = np.full(N, 0xDEADBEEF, np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    if nout is None:
        rc = lib.cufhe_amd_ps_test_vector(idx, values.ctypes.data_as(u32p), p, tv.ctypes.data_as(u32p))
    else:
        rc = lib.cufhe_amd_ps_test_vector_multi(idx, values.ctypes.data_as(u32p), p, nout, tv.ctypes.data_as(u32p))
    return rc, tv


@pytest.mark.parametrize("name", ["k2n512", "default"])
def test_test_vector_builders_equal_the_numpy_restatement(lib, name):
    idx, N = _set_index(lib, name)
    assert N == (512 if name == "k2n512" else 1024)
    rng = np.random.default_rng(N)
    for p in (2, 4, N // 2):
        v = rng.integers(0, 2**32, p, dtype=np.uint64).astype(np.uint32)
        rc, tv = _c_test_vector(lib, idx, N, v, p, None)
        assert rc == 0 and np.array_equal(tv, pc.test_vector(v, p, N)), f"{name}: p = {p}"
        assert tv[N - 1] == (0 - int(v[0])) & 0xFFFFFFFF and tv[0] == v[0], "the top half-box is -values[0]"
        for nout in (1, 2, 8):
            vv = rng.integers(0, 2**32, (nout, p), dtype=np.uint64).astype(np.uint32)
            rc, tv = _c_test_vector(lib, idx, N, vv, p, nout)
            if p * nout > N // 2:
                assert rc == -1 and np.all(tv == 0xDEADBEEF), f"{name}: p = {p}, nout = {nout} must be refused"
                continue
            assert rc == 0 and np.array_equal(tv, pc.test_vector_multi(vv, p, nout, N)), f"{name}: p = {p}, nout = {nout}"
            for j in range(nout):
                assert tv[N - nout + j] == (0 - int(vv[j][0])) & 0xFFFFFFFF and tv[j] == vv[j][0]
    v = np.arange(16, dtype=np.uint32)
    for p, nout in ((3, None), (6, None), (1, None), (N, None), (3, 2), (4, 3), (N // 2, 2), (N // 4, 4), (N // 8, 8)):
        rc, tv = _c_test_vector(lib, idx, N, np.resize(v, (nout or 1) * max(p, 1)), p, nout)
        assert rc == -1 and np.all(tv == 0xDEADBEEF), f"{name}: p = {p}, nout = {nout} must be refused"
    rc, _ = _c_test_vector(lib, lib.cufhe_amd_ps_count(), N, v, 4, None)
    assert rc == -1, "an unknown set must be refused"
    assert lib.cufhe_amd_ps_test_vector(idx, None, 4, None) == -1


# ---- the checker against the oracle ----
def test_smallmod_key_mapping_equals_the_c_function():
    L = ol.load_set("smallmod")
    L.orc_smallmod_from_torus.restype = ctypes.c_uint32
    L.orc_smallmod_from_torus.argtypes = [ctypes.c_uint32]
    a = np.concatenate([np.array([0, 1, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 2, 2**32 - 1], np.uint64),
                        np.random.default_rng(9).integers(0, 2**32, 2000, dtype=np.uint64)]).astype(np.uint32)
    want = np.array([L.orc_smallmod_from_torus(int(x)) for x in a], np.uint32)
    assert np.array_equal(pc.smallmod_from_torus(a), want)


@pytest.fixture(scope="module", params=ol.SETS)
def checker(request):
    return pc.Checker(request.param, seed=5)


def test_composition_equals_orc_blind_rotate(checker):
    """acc <- orc_cmux(BK_i, X^abar_i acc, acc) from the all-mu test vector is the oracle's blind rotation, after 0 to 3 steps"""
    C = checker
    rng = np.random.default_rng(11)
    tl = rng.integers(0, 2**32, size=(4, C.n + 1), dtype=np.uint64).astype(np.uint32)
    tl[0, :2] = 0
    tl[1, C.n] = 0                # bbar = 2N
    tl[2, C.n] = 0xFFFFFFFF       # bbar = 1
    tl[3, C.n] = 0x80000000       # bbar = N
    for steps in (0, 1, 2, 3):
        for g in range(4):
            assert np.array_equal(C.rotate(tl[g], None, 0, steps), C.K.blind_rotate(tl[g], steps)), f"{C.name}: input {g}, {steps} steps"
            assert np.array_equal(C.rotate(tl[g], C.mu_test_vector(), 0, steps), C.K.blind_rotate(tl[g], steps))


@pytest.mark.parametrize("level", [0, 1])
def test_composition_equals_orc_gate_batch_for_a_nand(checker, level):
    """the whole gate path of the checker -- lincomb, rotation, SampleExtract(0), key switch, in the order of the level -- with NAND's
    (-1, -1, mu) is orc_gate_batch's NAND"""
    C = checker
    a = C.K.encrypt(np.array([1], np.uint8), level, seed=70 + level)
    b = C.K.encrypt(np.array([0], np.uint8), level, seed=80 + level)
    got = C.user_gate_one(level, (-1, -1, 0), pc.MU, None, [a[0], b[0]])
    assert got.shape == (1, C.words[level])
    assert np.array_equal(got[0], C.K.gate_batch(NAND, level, a, b)[0]), f"{C.name}: level {level}"
    # SampleExtract at 0 of the checker is the oracle's
    acc = np.random.default_rng(5).integers(0, 2**32, C.acc_words, dtype=np.uint64).astype(np.uint32)
    t1 = np.zeros(C.words[1], np.uint32)
    C.L.orc_sample_extract0(t1, acc)
    assert np.array_equal(C.sample_extract(acc, 0), t1)


def test_rounded_modulus_switch(checker):
    """ms_abar / ms_bbar of cufhe_amd/csrc/kernels_common.hip.h:78-80 with the set's Nbit, restated in integers: abar is
    round(a 2N / 2^32 / 2^s) 2^s in 32-bit arithmetic (the sum wraps), bbar = 2N - floor(b 2N / 2^32 / 2^s) 2^s"""
    nbit, N = checker.nbit, checker.N
    for s in (0, 1, 2, 3):
        unit = 1 << (32 - 1 - nbit + s)              # torus words per multiple of 2^s of the 2N grid
        half = unit >> 1
        assert pc.ms_abar(0, s, nbit) == 0
        assert pc.ms_abar(2**32 - 1, s, nbit) == 0, "a + half wraps mod 2^32: X^2N = 1"
        assert pc.ms_abar(half - 1, s, nbit) == 0 and pc.ms_abar(half, s, nbit) == 1 << s, "the rounding boundary"
        assert pc.ms_abar(2**32 - half - 1, s, nbit) == 2 * N - (1 << s) and pc.ms_abar(2**32 - half, s, nbit) == 0
        assert pc.ms_abar(5 * unit + half, s, nbit) == 6 << s and pc.ms_abar(5 * unit + half - 1, s, nbit) == 5 << s
        assert pc.ms_bbar(0, s, nbit) == 2 * N and pc.ms_bbar(unit - 1, s, nbit) == 2 * N
        assert pc.ms_bbar(unit, s, nbit) == 2 * N - (1 << s)
        assert pc.ms_bbar(2**32 - 1, s, nbit) == 1 << s
        assert pc.ms_bbar(0x80000000, s, nbit) == N
    # s = 0 is the built-in gates' own switch (orc_blind_rotate: tests above)


def test_sample_extract_at_an_index(checker):
    """out_j[c N + m] = a_c[j - m] (m <= j), -a_c[N + j - m] (m > j); out_j[k N] = b[j]: the phase of out_j under the extracted key is
    coefficient j of the accumulator's phase polynomial -- checked directly on a noiseless TRLWE of a known polynomial"""
    C = checker
    N, k = C.N, C.k
    rng = np.random.default_rng(21)
    s1 = C.K.s1.reshape(k, N).astype(np.int64)
    a = rng.integers(0, 2**32, (k, N), dtype=np.uint64).astype(np.uint32)
    msg = rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32)
    b = msg.astype(np.uint64)
    for c in range(k):       # b = sum_c a_c s_c + msg, negacyclic, schoolbook on the key's set bits
        for i in np.flatnonzero(s1[c]):
            b = (b + pc.negacyclic_rotate(a[c], int(i)).astype(np.uint64) * np.uint64(s1[c][i])) & pc.M32
    acc = np.concatenate([a.reshape(-1), b.astype(np.uint32)])
    for j in (0, 1, 2, 7):
        t1 = C.sample_extract(acc, j)
        assert C.phase(1, t1[None, :])[0] == msg[j], f"{C.name}: SampleExtract({j})"
