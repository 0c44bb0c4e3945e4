"""User gates of the N = 2048 ring without a GPU: the checker against the oracle, the test-vector builder, a table gate under genuine
keys within the noise bounds INTEGRATION.md section 5.1 derives, and the C++ shim."""
import os
import subprocess

import numpy as np
import pytest

import lvl2_user_gate_checker as lc
import oracle_lib as ol

ROOT = ol.ROOT
n, N2 = ol.n, ol.N2


@pytest.fixture(scope="module")
def keys2(oracle, keys):
    return ol.KeysLvl2(oracle, keys, seed=7)


def _edge_inputs(rng, count):
    tl = rng.integers(0, 2**32, size=(count, n + 1), dtype=np.uint64).astype(np.uint32)
    tl[0, n] = 0                      # bbar = 2 N2: the identity
    tl[1, n] = 0x80000000             # bbar = N2
    tl[2, n] = 0xFFFFFFFF             # bbar = 1
    tl[2, :4] = 0
    return tl


@pytest.mark.parametrize("steps", [0, 1, 3, 630])
def test_checker_with_the_constant_tv_is_the_oracle_rotation(keys2, steps):
    """blind_rotate_tv with an all-2^61 test vector == orc2_blind_rotate, word for word, the edge cases of the first accumulator
    (bbar = 2 N2, N2, 1) among the inputs"""
    tl = _edge_inputs(np.random.default_rng(1400 + steps), 3 if steps == 630 else 4)
    got = lc.on_threads(lambda g: lc.blind_rotate_tv(keys2, tl[g], lc.mu_test_vector(), steps), tl.shape[0])
    for g in range(tl.shape[0]):
        assert np.array_equal(got[g], keys2.blind_rotate(tl[g], steps)), f"rotation {g} differs from orc2_blind_rotate after {steps} steps"


def test_checker_with_a_builtin_gates_coefficients_is_the_oracle_gate(keys, keys2):
    """(ca, cb, 0) and offset of NAND, XOR and ANDNY with TV None / all 2^61 give orc2_gate's words"""
    rng = np.random.default_rng(1410)
    bits = rng.integers(0, 2, (2, 3)).astype(np.uint8)
    a, b = keys.encrypt(bits[0], 0, seed=1411), keys.encrypt(bits[1], 0, seed=1412)
    cases = [("NAND", (-1, -1, 0), ol.MU, None), ("XOR", (2, 2, 0), 2 * ol.MU, lc.mu_test_vector()), ("ANDNY", (-1, 1, 0), -ol.MU, None)]
    got = lc.on_threads(lambda g: lc.user_gate_one(keys2, cases[g][1], cases[g][2], cases[g][3], [a[g], b[g]]), 3)
    want = keys2.gate_batch(np.array([ol.OPS.index(c[0]) for c in cases], np.int32), a, b)
    for g in range(3):
        assert np.array_equal(got[g], want[g]), f"{cases[g][0]} differs from orc2_gate"


def test_rotated_test_vector_edges():
    """the rule of the first accumulator at every edge: the identity at bbar = 2 N2, every word negated at N2, one wrap at 1"""
    tv = np.random.default_rng(1420).integers(0, 2**64, N2, dtype=np.uint64)
    neg = lambda v: (np.uint64(0) - v)      # noqa: E731
    with np.errstate(over="ignore"):
        assert np.array_equal(lc.rotated_tv(tv, 2 * N2), tv)
        assert np.array_equal(lc.rotated_tv(tv, N2), neg(tv))
        assert np.array_equal(lc.rotated_tv(tv, 1), np.concatenate([neg(tv[-1:]), tv[:-1]]))
        assert np.array_equal(lc.rotated_tv(tv, N2 + 1), np.concatenate([tv[-1:], neg(tv[:-1])]))
        assert np.array_equal(lc.rotated_tv(tv, 2 * N2 - 1), np.concatenate([tv[1:], neg(tv[:1])]))


@pytest.mark.parametrize("p", [2, 8, N2 // 2])
def test_test_vector_builder(p):
    """cufhe_amd_lvl2_test_vector: every box, the top half-box, the extremes p = 2 and p = N2 / 2; equal to the checker's restatement"""
    from cufhe_amd import api
    values = np.random.default_rng(p).integers(0, 2**64, p, dtype=np.uint64)
    tv = api.lvl2_test_vector(values)
    assert tv.dtype == np.uint64 and tv.shape == (N2,)
    box = N2 // p
    assert np.all(tv[:box // 2] == values[0])
    for m in range(1, p):
        assert np.all(tv[m * box - box // 2:m * box + box // 2] == values[m]), m
    assert np.all(tv[N2 - box // 2:] == np.uint64((-int(values[0])) % 2**64))
    assert np.array_equal(tv, lc.test_vector(values))


def test_test_vector_builder_refuses_bad_p():
    import ctypes
    import cufhe_amd._lib as _lib
    v = np.zeros(N2, np.uint64)
    for p in (0, 1, 3, 6, N2, 2 * N2, -4):
        assert _lib.lib.cufhe_amd_lvl2_test_vector(v.ctypes.data_as(ctypes.c_void_p), p, v.ctypes.data_as(ctypes.c_void_p)) == -1, p
    assert _lib.lib.cufhe_amd_lvl2_test_vector(None, 2, v.ctypes.data_as(ctypes.c_void_p)) == -1


def test_the_id_range_is_its_own():
    """the header's range lies above every other id range (capi.hip asserts the same at compile time)"""
    text = open(os.path.join(ROOT, "include", "cufhe_amd.h")).read()
    import re
    val = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))      # noqa: E731
    base = val("CUFHE_AMD_LVL2_USER_OP_BASE")
    assert base == lc.LVL2_USER_OP_BASE and val("CUFHE_AMD_LVL2_MAX_USER_GATES") == lc.LVL2_MAX_USER_GATES
    assert base > val("CUFHE_AMD_TL_CMUX_ROTATE_BASE") + 2 * ol.N - 1
    assert base > val("CUFHE_AMD_TL_SEIKS_AT_BASE") + ol.N - 1
    assert base >= val("CUFHE_AMD_USER_OP_BASE") + 8 * val("CUFHE_AMD_MAX_USER_GATES")


def test_table_gate_under_genuine_keys(keys, keys2):
    """A p = 8 table gate on all 8 messages, inputs encrypted at level 0 with sigma alpha0 = 2^-15: the lvl0 output decrypts to f(m),
    and the lvl2 output's phase is within six sigma (derived, section 5.1: lc.noise_sigmas) of f(m)'s 64-bit word.  The sampled
    figures are printed; profiles/r14_lvl2_user_gates.md records them."""
    import user_gate_checker as uc
    p = 8
    s2, s0, rotation, keyswitch = lc.noise_sigmas()
    assert abs(rotation - 7.40e-16) < 0.01e-16 and abs(keyswitch - 1.033e-5) < 0.001e-5      # the figures INTEGRATION.md quotes
    assert 6 * s0 < 1.0 / (4 * p)           # the lvl0 output stays inside half a box of the p-ary encoding
    rng = np.random.default_rng(1430)
    f = rng.permutation(p)
    # f(m) in the padded p-ary encoding, with low bits that only the lvl2 output can show
    values = (f.astype(np.uint64) << np.uint64(60)) + rng.integers(0, 2**20, p, dtype=np.uint64)
    tv = lc.test_vector(values)
    step = (1 << 32) // (2 * p)
    ins = uc.encrypt_torus(keys, 0, np.arange(p, dtype=np.uint64) * np.uint64(step), 2.0 ** -15 * 2.0 ** 32, seed=1431)
    t2 = lc.on_threads(lambda m: lc.user_extract_one(keys2, (1, 0, 0), 0, tv, [ins[m]]), p)
    err2 = np.array([lc.signed64(np.uint64((int(keys2.phase2(t2[m])) - int(values[m])) % 2**64)) for m in range(p)])
    out0 = np.stack([keys2.keyswitch(t2[m]) for m in range(p)])
    ph0 = uc.phase(keys, 0, out0).astype(np.int64)
    err0 = ((ph0 - (values >> np.uint64(32)).astype(np.int64) + 2**31) % 2**32 - 2**31) / 2.0 ** 32
    print(f"lvl2 output: sampled std {err2.std():.3e}, max |err| {np.abs(err2).max():.3e}, derived sigma {s2:.3e}, bound {6 * s2:.3e}")
    print(f"lvl0 output: sampled std {err0.std():.3e}, max |err| {np.abs(err0).max():.3e}, derived sigma {s0:.3e}, bound {6 * s0:.3e}")
    assert np.abs(err2).max() < 6 * s2, (err2, s2)
    assert np.abs(err0).max() < 6 * s0, (err0, s0)
    dec = np.rint(ph0 / float(step)).astype(np.int64) % (2 * p)      # f(m) sits at f(m) 2^32 / (2p)
    assert np.array_equal(dec, f), (dec, f)


def test_shim_compiles_with_the_new_names(tmp_path):
    """include/cufhe_amd.hpp: DefineGateLvl2 / TestVectorLvl2 and Apply / gApply on the handle, plain g++"""
    src = tmp_path / "user.cpp"
    src.write_text('''#include "cufhe_amd.hpp"
void user(cufhe::Ctxt<TFHEpp::lvl0param>& out, cufhe::Ctxt<TFHEpp::lvl0param>& a, cufhe::Ctxt<TFHEpp::lvl0param>& b,
          cufhe::Ctxt<TFHEpp::lvl0param>& c, cufhe::Stream st) {
    std::vector<uint64_t> values(8);
    for (int m = 0; m < 8; m++) values[m] = (uint64_t)(7 - m) << 60;
    std::vector<uint64_t> tv = cufhe::TestVectorLvl2(values);
    cufhe::UserGate g = cufhe::DefineGateLvl2({1, 0, 0}, 0u, tv.data());
    cufhe::UserGate maj = cufhe::DefineGateLvl2({1, 1, 1}, 0u);
    static_assert(CUFHE_AMD_LVL2_USER_OP_BASE > CUFHE_AMD_TL_CMUX_ROTATE(2047), "own id range");
    cufhe::Apply(g, out, a, st);
    cufhe::gApply(maj, out, a, b, c, st);
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
