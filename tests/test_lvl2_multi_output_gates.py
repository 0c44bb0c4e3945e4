"""Multi-output gates of the N = 2048 ring and the one-rotation circuit bootstrap without a GPU: the checker
(tests/lvl2_multi_checker.py) against the single-output checkers it is built on, the interleaved test-vector builder, the header's
macros and id range, and the one-rotation stage 1 under genuine keys within the six-sigma bound of INTEGRATION.md section 5.1."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cb_checker as cb
import lvl2_multi_checker as mc
import lvl2_user_gate_checker as lc
import oracle_lib as ol

ROOT = ol.ROOT
n, N2 = ol.n, ol.N2


@pytest.fixture(scope="module")
def keys2(oracle, keys):
    return ol.KeysLvl2(oracle, keys, seed=7)


def _inputs(seed, count):
    tl = np.random.default_rng(seed).integers(0, 2**32, size=(count, n + 1), dtype=np.uint64).astype(np.uint32)
    tl[0, n] = 0                      # bbar = 2 N2: the identity
    tl[1, n] = 0x80000000             # bbar = N2
    tl[1, :4] = [0, 0x7FFFFFFF, 0xFFFFFFFF, 0xFFF80000]
    return tl


@pytest.mark.parametrize("steps", [0, 1, 3])
def test_checker_at_s0_is_the_single_output_checker(keys2, steps):
    tl = _inputs(1800 + steps, 3)
    tv = np.random.default_rng(1810).integers(0, 2**64, N2, dtype=np.uint64)
    coeffs, off = (3, -2, 0), 0x12345678
    for g in range(3):
        got = mc.multi_rotate_one(keys2, coeffs, off, tv, 1, [tl[g], tl[(g + 1) % 3]], steps)
        want = lc.user_rotate_one(keys2, coeffs, off, tv, [tl[g], tl[(g + 1) % 3]], steps)
        assert np.array_equal(got, want), (g, steps)
        assert np.array_equal(mc.sample_extract(got, 0), keys2.sample_extract(want)), "SampleExtract(0) is orc2_sample_extract0"


def test_checker_at_s0_with_a_constant_tv_is_blind_rotate_mu(keys2):
    tl = _inputs(1820, 2)
    for g, r in ((0, 0), (1, 2)):
        mu = cb.cb_mu(r)
        got = mc.blind_rotate_tv_multi(keys2, tl[g], np.full(N2, mu, np.uint64), 0, steps=2)
        assert np.array_equal(got, cb.blind_rotate_mu(keys2, tl[g], mu, steps=2)), (g, r)


def test_rounded_modulus_switch():
    """abar and bbar are multiples of 2^s within 2^(s-1) (a: rounded) resp. 2^s (b: truncated) of the plain ones; s = 0 is the plain switch"""
    rng = np.random.default_rng(1830)
    words = np.concatenate([rng.integers(0, 2**32, 200, dtype=np.uint64), [0, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 0xFFF80000, (1 << 20) - 1]])
    for w in words:
        w = int(w)
        assert mc.ms_abar(w, 0) == ((w + (1 << 19)) & 0xFFFFFFFF) >> 20 and mc.ms_bbar(w, 0) == 2 * N2 - (w >> 20)
        for s in (1, 2, 3):
            a, b = mc.ms_abar(w, s), mc.ms_bbar(w, s)
            assert a % (1 << s) == 0 and b % (1 << s) == 0 and 0 <= a < 2 * N2 and 1 <= b <= 2 * N2
            d = (a * (1 << 20) - w + 2**31) % 2**32 - 2**31
            assert abs(d) <= 1 << (19 + s), (w, s)
            assert 0 <= (2 * N2 - b) * (1 << 20) <= w < (2 * N2 - b + (1 << s)) * (1 << 20)


def test_sample_extract_index_is_a_coefficient_of_the_phase():
    """the phase of SampleExtract(j) under a key s is coefficient j of b - a s in Z[X]/(X^N2 + 1)"""
    rng = np.random.default_rng(1840)
    acc = rng.integers(0, 2**64, 2 * N2, dtype=np.uint64)
    key = rng.integers(0, 2, N2).astype(object)
    a = [int(x) for x in acc[:N2]]
    for j in (0, 1, 3, 7):
        t = mc.sample_extract(acc, j)
        ph = (int(t[N2]) - sum(int(t[m]) * int(key[m]) for m in range(N2))) % 2**64
        want = int(acc[N2 + j])
        for m in range(N2):
            if key[m]:
                want -= a[j - m] if m <= j else -a[N2 + j - m]
        assert ph == want % 2**64, j


@pytest.mark.parametrize("p,nout", [(2, 1), (4, 2), (4, 4), (2, 8), (128, 8)])
def test_test_vector_multi_builder(p, nout):
    from cufhe_amd import api
    values = np.random.default_rng(100 * p + nout).integers(0, 2**64, (nout, p), dtype=np.uint64)
    tv = api.lvl2_test_vector_multi(values)
    assert tv.dtype == np.uint64 and tv.shape == (N2,)
    assert np.array_equal(tv, mc.test_vector_multi(values))
    if nout == 1:
        assert np.array_equal(tv, api.lvl2_test_vector(values[0])) and np.array_equal(tv, lc.test_vector(values[0]))
    # output j at a position 0 mod nout reads values[j] of the position's box; the top half-box is negated
    assert all(tv[j] == values[j][0] for j in range(nout))
    assert all(tv[N2 - nout + j] == np.uint64((-int(values[j][0])) % 2**64) for j in range(nout))


def test_test_vector_multi_builder_refusals():
    import cufhe_amd._lib as _lib
    v = np.zeros(8 * N2, np.uint64)
    t = np.zeros(N2, np.uint64)
    f = _lib.lib.cufhe_amd_lvl2_test_vector_multi
    vp, tp = v.ctypes.data_as(ctypes.c_void_p), t.ctypes.data_as(ctypes.c_void_p)
    for p, nout in ((N2 // 2, 2), (256, 8), (N2, 1), (3, 2), (6, 1), (4, 3), (4, 16), (1, 2), (0, 2), (4, 0), (-4, 2)):
        assert f(vp, p, nout, tp) == -1, (p, nout)
    assert f(None, 4, 2, tp) == -1 and f(vp, 4, 2, None) == -1
    assert f(vp, N2 // 16, 8, tp) == 0 and f(vp, N2 // 2, 1, tp) == 0


def test_header_macros_and_id_range():
    text = open(os.path.join(ROOT, "include", "cufhe_amd.h")).read()
    val = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))      # noqa: E731
    assert val("CUFHE_AMD_LVL2_USER_OP_BASE") == mc.LVL2_USER_OP_BASE and val("CUFHE_AMD_LVL2_MAX_USER_GATES") == mc.LVL2_MAX_USER_GATES
    assert re.search(r"#define CUFHE_AMD_LVL2_USER_OP_OUTPUT\(op, j\) \(\(op\) \+ \(j\) \* CUFHE_AMD_LVL2_MAX_USER_GATES\)", text)
    assert mc.user_op_output(mc.LVL2_USER_OP_BASE + 63, 7) == mc.LVL2_USER_OP_LAST == 8703
    from cufhe_amd import api
    assert api.lvl2_user_op_output(8200, 3) == mc.user_op_output(8200, 3) == 8392
    assert "cufhe_amd_lvl2_define_gate_multi(" in text and "cufhe_amd_lvl2_test_vector_multi(" in text and '"cb_rotations"' in text
    lib = ctypes.CDLL(os.path.join(ROOT, "cufhe_amd", "libcufhe_amd.so"))
    assert hasattr(lib, "cufhe_amd_lvl2_define_gate_multi") and hasattr(lib, "cufhe_amd_lvl2_test_vector_multi")


def test_the_snippet_of_section_5_2_compiles(tmp_path):
    """the C snippet of INTEGRATION.md section 5.2 (the first ```c block after the section's heading) against the header, plain gcc"""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("### 5.2"):]
    code = re.search(r"```c\n(.*?)```", sec, re.S).group(1)
    assert "cufhe_amd_lvl2_define_gate_multi" in code and "CUFHE_AMD_LVL2_USER_OP_OUTPUT" in code
    src = tmp_path / "snippet.c"
    src.write_text('#include "cufhe_amd.h"\n' + code)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_shim_compiles_with_the_multi_output_names(tmp_path):
    src = tmp_path / "user.cpp"
    src.write_text('''#include "cufhe_amd.hpp"
void user(cufhe::Ctxt<TFHEpp::lvl0param>& sum, cufhe::Ctxt<TFHEpp::lvl0param>& carry, cufhe::Ctxt<TFHEpp::lvl0param>& a,
          cufhe::Ctxt<TFHEpp::lvl0param>& b, cufhe::Ctxt<TFHEpp::lvl0param>& c, cufhe::Stream st) {
    std::vector<std::vector<uint64_t>> values(2, std::vector<uint64_t>(4));
    std::vector<uint64_t> tv = cufhe::TestVectorMultiLvl2(values, 4);
    cufhe::UserGate g = cufhe::DefineGateLvl2({1, 1, 1}, 0u, tv.data(), 2);
    static_assert(CUFHE_AMD_LVL2_USER_OP_OUTPUT(CUFHE_AMD_LVL2_USER_OP_BASE + 63, 7) == 8703, "id range");
    cufhe::gApply(cufhe::Output(g, 0), sum, a, b, c, st);
    cufhe::gApply(cufhe::Output(g, 1), carry, a, b, c, st);
}
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_one_rotation_stage_1_under_genuine_keys(keys, keys2):
    """4 inputs, both bit values: row r of the checker's one-rotation stage 1 decrypts under s2 to bit * 2^(64 - 6 (r + 1)), the error
    below six sigma of the rotation (lc.noise_sigmas: the blind-rotation noise does not depend on the test vector)"""
    bits = np.array([0, 1, 1, 0], np.uint8)
    ins = keys.encrypt(bits, 0, seed=1850)
    stage1 = mc.cb_rotate_batch(keys2, ins)
    assert stage1.shape == (4, cb.CB_L, cb.PKS_IN)
    s2 = lc.noise_sigmas()[0]
    errs = []
    for g in range(4):
        for r in range(cb.CB_L):
            want = int(bits[g]) << (64 - cb.CB_BGBIT * (r + 1))
            errs.append(float(lc.signed64(np.uint64((int(keys2.phase2(stage1[g, r])) - want) % 2**64))))
    errs = np.array(errs)
    print(f"one-rotation stage 1: sampled std {errs.std():.3e}, max |err| {np.abs(errs).max():.3e}, derived sigma {s2:.3e}, bound {6 * s2:.3e}")
    assert np.abs(errs).max() < 6 * s2, (errs, s2)
