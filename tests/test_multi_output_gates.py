"""CPU tests of multi-output user gates (cufhe_amd_define_gate_multi): the numpy checker of tests/multi_output_checker.py against the
single-output checker and the phase algebra of SampleExtract(j), the interleaved test-vector helper, and the refusals of the C ABI
that need no device."""
import ctypes

import numpy as np
import pytest

import multi_output_checker as mc
import oracle_lib as ol
import user_gate_checker as uc

U32P = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def keys():
    return ol.Keys(ol.load(), seed=13)


@pytest.fixture(scope="module")
def eng():
    import cufhe_amd
    return cufhe_amd


@pytest.mark.parametrize("level", [0, 1])
def test_checker_with_one_output_is_the_user_gate_checker(keys, level):
    """nout = 1 (s = 0), j = 0: the single-output checker word for word (which tests/test_user_gates.py ties to orc_gate)"""
    rng = np.random.default_rng(40 + level)
    ins = [rng.integers(0, 1 << 32, size=ol.LVL_WORDS[level], dtype=np.uint64).astype(np.uint32) for _ in range(2)]
    tv = rng.integers(0, 1 << 32, size=ol.N, dtype=np.uint64).astype(np.uint32)
    got = mc.multi_gate_one(keys, level, (1, -1, 0), 0x12345678, tv, 1, ins)
    assert len(got) == 1
    assert np.array_equal(got[0], uc.user_gate_one(keys, level, (1, -1, 0), 0x12345678, tv, ins))


def test_sample_extract_j_phase_is_coefficient_j(keys):
    """for random accumulators, the phase of SampleExtract(j) under the lvl1 key is coefficient j of the accumulator's phase
    b - a s mod (X^N + 1, 2^32), exactly"""
    rng = np.random.default_rng(7)
    s = keys.key(1).astype(np.int64)
    N = ol.N
    for _ in range(3):
        acc = rng.integers(0, 1 << 32, size=2 * N, dtype=np.uint64).astype(np.uint32)
        a = acc[:N].astype(np.int64)
        full = np.convolve(a, s)                             # |a s| < N 2^32: exact in int64
        prod = full[:N].copy()
        prod[:N - 1] -= full[N:]
        ph = (acc[N:].astype(np.int64) - prod) % (1 << 32)
        for j in (0, 1, 2, 3, 7, 100, N - 1):
            t = mc.sample_extract(acc, j)
            assert int(uc.phase(keys, 1, t)[0]) == int(ph[j]), f"coefficient {j}"


def test_modulus_switch_with_s_zero_is_the_gates_rounding():
    rng = np.random.default_rng(3)
    for a in rng.integers(0, 1 << 32, size=200, dtype=np.uint64):
        assert mc.ms_abar(int(a), 0) == uc.mod_switch((int(a) + (1 << (32 - 2 - uc.NBIT))) & 0xFFFFFFFF)
        assert mc.ms_bbar(int(a), 0) == 2 * ol.N - uc.mod_switch(int(a))
        for s in (1, 2, 3):
            assert mc.ms_abar(int(a), s) % (1 << s) == 0 and mc.ms_bbar(int(a), s) % (1 << s) == 0


def test_test_vector_multi_one_output_is_test_vector(eng):
    rng = np.random.default_rng(5)
    for p in (2, 4, 8, 64, 512):
        v = rng.integers(0, 1 << 32, size=p, dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(eng.test_vector_multi(v[None, :]), eng.test_vector(v))


@pytest.mark.parametrize("nout", [2, 4, 8])
def test_test_vector_multi_matches_numpy(eng, nout):
    rng = np.random.default_rng(nout)
    for p in (2, 4, 8, 512 // nout):
        v = rng.integers(0, 1 << 32, size=(nout, p), dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(eng.test_vector_multi(v), mc.test_vector_multi(v)), (nout, p)


def test_test_vector_multi_refusals(eng):
    lib = eng.lib
    tv = np.zeros(ol.N, np.uint32)
    vals = np.zeros(8 * 1024, np.uint32)
    for p, nout in ((4, 3), (4, 0), (4, 16), (4, -2), (3, 2), (1, 2), (0, 2), (512, 2), (128, 8), (256, 4)):
        rc = lib.cufhe_amd_test_vector_multi(vals.ctypes.data_as(U32P), p, nout, tv.ctypes.data_as(U32P))
        assert rc == -1, (p, nout)
    assert lib.cufhe_amd_test_vector_multi(None, 4, 2, tv.ctypes.data_as(U32P)) == -1
    assert lib.cufhe_amd_test_vector_multi(vals.ctypes.data_as(U32P), 4, 2, None) == -1
    # the largest allowed: p nout = N / 2
    assert lib.cufhe_amd_test_vector_multi(vals.ctypes.data_as(U32P), 64, 8, tv.ctypes.data_as(U32P)) == 0


def test_define_gate_multi_refusals_without_a_device(eng):
    lib = eng.lib
    op = ctypes.c_int(-7)
    coeffs = (ctypes.c_int32 * 3)(1, 1, 1)
    tv = np.zeros(ol.N, np.uint32)
    tvp = tv.ctypes.data_as(U32P)
    for nout in (0, 1, 3, 16, -2):
        rc = lib.cufhe_amd_define_gate_multi(coeffs, 0, nout, tvp, ctypes.byref(op))
        assert rc == -1 and b"nout" in lib.cufhe_amd_last_error()
    rc = lib.cufhe_amd_define_gate_multi(coeffs, 0, 2, None, ctypes.byref(op))
    assert rc == -1 and b"test vector" in lib.cufhe_amd_last_error()
    rc = lib.cufhe_amd_define_gate_multi((ctypes.c_int32 * 3)(0, 1, 1), 0, 2, tvp, ctypes.byref(op))
    assert rc == -1 and b"c0" in lib.cufhe_amd_last_error()
    rc = lib.cufhe_amd_define_gate_multi(coeffs, 0, 4, tvp, ctypes.byref(op))
    assert rc == -3 and b"Initialize" in lib.cufhe_amd_last_error() and op.value == -7
    with pytest.raises(eng.CufheAmdError):
        eng.define_gate((1, 1, 1), 0, tv, nout=2)


def test_output_ids_are_checked_without_a_device(eng):
    lib = eng.lib
    base, cap = eng.USER_OP_BASE, eng.MAX_USER_GATES
    assert eng.user_op_output(base + 5, 0) == base + 5 and eng.user_op_output(base + 63, 7) == base + 8 * cap - 1 < 1512
    for op in (eng.user_op_output(base, 1), eng.user_op_output(base + cap - 1, 7)):
        rc = lib.cufhe_amd_gate(0, None, op, 0, None, None, None, None)
        assert rc == -1 and b"unknown gate op" in lib.cufhe_amd_last_error()
        ops = np.array([eng.NAND, op], np.int32)
        rc = lib.cufhe_amd_gate_list(0, None, 0, 2, ops.ctypes.data, (ctypes.c_void_p * 2)(8, 8), (ctypes.c_void_p * 2)(8, 8),
                                     None, None)
        assert rc == -1 and b"unknown gate op" in lib.cufhe_amd_last_error()
        rc = lib.cufhe_amd_enqueue_gate(0, None, op, 0, None, None, None, None)
        assert rc == -1 and b"unknown gate op" in lib.cufhe_amd_last_error()
    # the multi-output entry point takes only a defined multi-output op
    outs = (ctypes.c_void_p * 2)(8, 16)
    rc = lib.cufhe_amd_enqueue_gate_multi(0, None, base, 0, 2, outs, None, None, None)
    assert rc == -1 and b"not defined" in lib.cufhe_amd_last_error()
    rc = lib.cufhe_amd_enqueue_gate_multi(0, None, eng.NAND, 0, 2, outs, None, None, None)
    assert rc == -1 and b"multi-output" in lib.cufhe_amd_last_error()


def test_cpp_program_compiles():
    """tests/cpp/test_multi_output_gates.cpp (DefineGate(.., nout) / TestVectorMulti / ApplyMulti / gApplyMulti) builds with plain g++"""
    import os
    import subprocess
    import cpp_build
    cdefs, libs = cpp_build.hip_flags()
    root = ol.ROOT
    exe = os.path.join(root, "tests", "cpp", "test_multi_output_gates")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + cdefs +
                          ["-o", exe, os.path.join(root, "tests", "cpp", "test_multi_output_gates.cpp"),
                           "-L" + os.path.join(root, "cufhe_amd"), "-lcufhe_amd", "-L" + os.path.join(root, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(root, "cufhe_amd"), "-Wl,-rpath," + os.path.join(root, "oracle")] + libs)
    assert os.path.exists(exe)
