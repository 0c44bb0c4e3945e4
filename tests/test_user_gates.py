"""CPU tests of user gates (cufhe_amd_define_gate): the composed checker of tests/user_gate_checker.py against orc_gate, the
test-vector helper's boxes and signs, and the refusals of the C ABI that need no device."""
import ctypes
import time

import numpy as np
import pytest

import oracle_lib as ol
import user_gate_checker as uc

OPS = {name: i for i, name in enumerate(ol.OPS)}


@pytest.fixture(scope="module")
def keys():
    L = ol.load()
    return ol.Keys(L, seed=11)


def gate_coeffs(L, op):
    ca, cb, om = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    L.orc_gate_coeffs(op, ctypes.byref(ca), ctypes.byref(cb), ctypes.byref(om))
    return ca.value, cb.value, (om.value * ol.MU) & 0xFFFFFFFF


@pytest.mark.parametrize("level,names", [(0, ("NAND", "XOR", "ORYN")), (1, ("AND", "XNOR", "ANDNY"))])
def test_composed_checker_reproduces_orc_gate(keys, level, names):
    """blind rotation rebuilt from orc_cmux steps with the mu test vector == the oracle's own gate, word for word"""
    rng = np.random.default_rng(5 + level)
    count = 2
    for name in names:
        op = OPS[name]
        bits = rng.integers(0, 2, size=(2, count)).astype(np.uint8)
        a = keys.encrypt(bits[0], level, seed=300 + op)
        b = keys.encrypt(bits[1], level, seed=400 + op)
        ca, cb, off = gate_coeffs(keys.L, op)
        t = time.time()
        got = uc.user_gate_batch(keys, level, (ca, cb, 0), off, None, [a, b])
        want = keys.gate_batch(op, level, a, b)
        assert np.array_equal(got, want), f"{name} level {level}: composed checker differs from orc_gate"
        # an explicit all-mu vector is the same thing
        assert np.array_equal(uc.user_gate_one(keys, level, (ca, cb, 0), off, uc.mu_test_vector(), [a[0], b[0]]), want[0])
        assert time.time() - t < 120


@pytest.fixture(scope="module")
def eng():
    import cufhe_amd
    return cufhe_amd


@pytest.mark.parametrize("p", [2, 4, 8, 16, 32, 64, 128, 256, 512])
def test_test_vector_boxes_and_signs(eng, p):
    """X^-j TV at coefficient 0 (the negacyclic lookup of a bootstrap at phase j / 2N) is values[m(j)] for every j of the
    padded half of the torus, m(j) the message nearest to j"""
    rng = np.random.default_rng(p)
    values = rng.integers(0, 1 << 32, size=p, dtype=np.uint64).astype(np.uint32)
    tv = eng.test_vector(values)
    N = ol.N
    box = N // p
    for j in range(-box // 2, N - box // 2):
        k = j % (2 * N)
        got = tv[k] if k < N else (0 - int(tv[k - N])) & 0xFFFFFFFF
        m = (j + box // 2) // box
        assert got == values[m], (p, j, m)
    # boxes: the top half-box holds -values[0]
    assert all(tv[N - 1 - i] == (0 - int(values[0])) & 0xFFFFFFFF for i in range(box // 2))


def test_test_vector_refusals(eng):
    lib = eng.lib
    tv = np.zeros(ol.N, np.uint32)
    vals = np.zeros(1024, np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    for p in (0, 1, 3, 6, 1024, -2):
        rc = lib.cufhe_amd_test_vector(vals.ctypes.data_as(u32p), p, tv.ctypes.data_as(u32p))
        assert rc == -1 and b"power of two" in lib.cufhe_amd_last_error()
    assert lib.cufhe_amd_test_vector(None, 4, tv.ctypes.data_as(u32p)) == -1


def test_define_gate_refusals_without_a_device(eng):
    lib = eng.lib
    i32p = ctypes.POINTER(ctypes.c_int32)
    op = ctypes.c_int(-7)
    coeffs = (ctypes.c_int32 * 3)(1, 1, 1)
    # before Initialize
    rc = lib.cufhe_amd_define_gate(coeffs, 0, None, ctypes.byref(op))
    assert rc == -3 and b"Initialize" in lib.cufhe_amd_last_error() and op.value == -7
    # all-zero coefficients, c0 = 0, null arguments: refused before anything else
    for c in ((0, 0, 0), (0, 1, 1)):
        rc = lib.cufhe_amd_define_gate((ctypes.c_int32 * 3)(*c), 0, None, ctypes.byref(op))
        assert rc == -1 and b"c0" in lib.cufhe_amd_last_error()
    assert lib.cufhe_amd_define_gate(ctypes.cast(None, i32p), 0, None, ctypes.byref(op)) == -1
    assert lib.cufhe_amd_define_gate(coeffs, 0, None, None) == -1
    with pytest.raises(eng.CufheAmdError):
        eng.define_gate((1, 1, 1))


def test_user_op_ids_are_checked_without_a_device(eng):
    lib = eng.lib
    base, cap = eng.USER_OP_BASE, eng.MAX_USER_GATES
    assert base > max(len(ol.OPS), 103)                     # past enum cufhe_amd_op and enum cufhe_amd_trlwe_op
    # an id of the range that has no definition: refused by the batch entry points before any device work
    for op in (base, base + cap - 1):
        rc = lib.cufhe_amd_gate(0, None, op, 0, None, None, None, None)
        assert rc == -1 and b"not defined" in lib.cufhe_amd_last_error()
        ops = np.array([eng.NAND, op], np.int32)
        rc = lib.cufhe_amd_gate_list(0, None, 1, 2, ops.ctypes.data, (ctypes.c_void_p * 2)(8, 8), (ctypes.c_void_p * 2)(8, 8),
                                     None, None)
        assert rc == -1 and b"not defined" in lib.cufhe_amd_last_error()
    # the per-gate API checks the id first: undefined and out-of-range ids
    rc = lib.cufhe_amd_enqueue_gate(0, None, base, 0, None, None, None, None)
    assert rc == -1 and b"not defined" in lib.cufhe_amd_last_error()
    for op in (base + cap, base - 1, -1):
        rc = lib.cufhe_amd_enqueue_gate(0, None, op, 0, None, None, None, None)
        assert rc == -1 and b"unknown gate op" in lib.cufhe_amd_last_error()


def test_cpp_program_compiles():
    """tests/cpp/test_user_gates.cpp (DefineGate / TestVector / Apply / gApply of include/cufhe_amd.hpp) builds with plain g++; it runs in
    tests/test_gpu_user_gates.py"""
    import os
    assert os.path.exists(uc.build_cpp_program())
