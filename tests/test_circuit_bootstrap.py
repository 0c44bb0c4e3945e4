"""Circuit bootstrapping without a GPU: the checker's lvl02 rotation against the oracle, the digits of the private key switch,
the C ABI and the C++ shim."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cb_checker as cb
import oracle_lib as ol

ROOT = ol.ROOT


@pytest.fixture(scope="module")
def keys2(oracle, keys):
    return ol.KeysLvl2(oracle, keys, seed=7)


def test_checker_rotation_is_the_oracle_at_the_default_mu(keys2):
    """blind_rotate_mu + sample extract at mu = 2^61 == orc2_blind_rotate + orc2_sample_extract0, word for word (full 630 steps, and
    the edge cases of the rotated test vector: bbar = 2N, bbar = N, abar = 0)"""
    rng = np.random.default_rng(31)
    tl = rng.integers(0, 2**32, size=(3, ol.n + 1), dtype=np.uint64).astype(np.uint32)
    tl[0, :5] = 0
    tl[1, ol.n] = 0
    tl[2, ol.n] = 0x80000000
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(3) as ex:
        got = list(ex.map(lambda g: keys2.sample_extract(cb.blind_rotate_mu(keys2, tl[g], ol.MU2)), range(3)))
    for g in range(3):
        want = keys2.sample_extract(keys2.blind_rotate(tl[g]))
        assert np.array_equal(got[g], want), f"checker rotation {g} differs from orc2_blind_rotate"


def test_checker_rotation_scales_with_mu(keys2):
    """a few steps at mu_r: the rotated test vector carries +-mu_r, and a trivial ciphertext (a = 0) decrypts to +-mu_r exactly"""
    tl = np.zeros(ol.n + 1, np.uint32)
    tl[ol.n] = 1 << 29                        # phase 1/8: +mu
    for r in range(cb.CB_L):
        acc = cb.blind_rotate_mu(keys2, tl, cb.cb_mu(r), steps=ol.n)
        t2 = keys2.sample_extract(acc)
        ph = int(keys2.phase2(t2))
        err = (ph - cb.cb_mu(r) + 2**63) % 2**64 - 2**63
        assert abs(err) < 2**40, (r, err)


def test_private_keyswitch_digits_recombine():
    """sum_j a_ij 2^(64 - 3 (j + 1)) is abar_i rounded to 30 bits: within 2^33 of tlwe2[i]"""
    rng = np.random.default_rng(5)
    t2 = rng.integers(0, 2**64, size=cb.PKS_IN, dtype=np.uint64)
    t2[0] = 0
    t2[1] = np.uint64(2**64 - 1)
    ii, jj, vv = cb.pks_digits(t2)
    rec = np.zeros(cb.PKS_IN, dtype=object)
    for i, j, v in zip(ii, jj, vv):
        rec[i] += int(v) << (64 - 3 * (int(j) + 1))
    for i in range(cb.PKS_IN):
        d = (int(t2[i]) - rec[i] + 2**63) % 2**64 - 2**63
        assert -2**33 <= d < 2**33, (i, d)
    assert not np.any(ii == 0), "the zero word has no nonzero digit"


def test_private_keyswitch_gather_is_the_definition():
    """the numpy gather-sum == a plain loop over the definition, on a key whose rows are known (a view: no 2.35 GB)"""
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 2**32, size=(2, 97, 2 * ol.N), dtype=np.uint64).astype(np.uint32)
    idx = np.arange(cb.PKS_IN * cb.PKS_T * cb.PKS_NUMBASE) % 97
    key = rows[:, idx, :]                                  # [2][rows][2N]: 2 x 143 430 x 2048 words would be the full key
    t2 = rng.integers(0, 2**64, size=cb.PKS_IN, dtype=np.uint64)
    got = cb.private_keyswitch_one(key, t2).reshape(2, 2 * ol.N)
    ii, jj, vv = cb.pks_digits(t2)
    want = np.zeros((2, 2 * ol.N), np.uint64)
    for i, j, v in zip(ii, jj, vv):
        r = idx[(i * cb.PKS_T + j) * cb.PKS_NUMBASE + v - 1]
        want -= rows[:, r, :].astype(np.uint64)
    assert np.array_equal(got, (want & np.uint64(0xFFFFFFFF)).astype(np.uint32))


def test_c_abi_symbols_and_header():
    so = os.path.join(ROOT, "cufhe_amd", "libcufhe_amd.so")
    lib = ctypes.CDLL(so)
    names = ("cufhe_amd_cb_get_params", "cufhe_amd_cb_initialize", "cufhe_amd_cb_rotate_batch", "cufhe_amd_private_keyswitch_batch",
             "cufhe_amd_circuit_bootstrap_batch")
    hdr = open(os.path.join(ROOT, "include", "cufhe_amd.h")).read()
    for nm in names:
        assert hasattr(lib, nm), nm
        assert nm + "(" in hdr, nm
    assert "CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP = 104" in hdr
    import cufhe_amd
    p = cufhe_amd.api.cb_params()           # needs no device
    assert (p.n, p.N, p.k, p.l, p.Bgbit, p.N2, p.l2, p.Bgbit2, p.t, p.basebit) == (630, 1024, 1, 3, 6, 2048, 4, 9, 10, 3)
    assert p.privksk_words == cb.PKS_KEY_WORDS == 587489280
    assert p.trgsw_words == cb.TRGSW_WORDS and p.trgsw_ntt_doubles == cb.TRGSW_WORDS and p.lvl2_words == cb.PKS_IN


def test_cpp_shim_circuit_bootstrapping_compiles(tmp_path):
    src = tmp_path / "cb.cpp"
    src.write_text('#include "cufhe_amd.hpp"\n'
                   'void f(const uint32_t* k, size_t w, cufhe::Stream st) {\n'
                   '    cufhe::InitializeCircuitBootstrapping(k, w);\n'
                   '    cufhe::Ctxt<TFHEpp::lvl0param> in;\n'
                   '    cufhe::cuFHETRGSWNTTlvl1 sel;\n'
                   '    cufhe::cuFHETRLWElvl1 res, c1, c0;\n'
                   '    cufhe::CircuitBootstrapping(sel, in, st);\n'
                   '    cufhe::gCircuitBootstrapping(sel, in, st);\n'
                   '    cufhe::gCMUXNTT(res, sel, c1, c0, st);\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
