"""CPU tests of tests/exponent_sweep.py, the reference of the GPU exponent sweep: the edge words by brute force, X^e p against
schoolbook multiplication by the monomial, and -- for EVERY exponent -- agreement with the helpers the rest of the suite relies on
and with the oracles' own first accumulators.  Two references that disagree would be a finding; they do not."""
import numpy as np
import pytest

import cb_checker as cb
import exponent_sweep as es
import lut_checker as lc
import lvl2_multi_checker as m2
import lvl2_user_gate_checker as l2
import multi_output_checker as mc
import oracle_lib as ol
import packed_rom_checker as pr
import ps_user_gate_checker as pc
import user_gate_checker as uc

NBITS, SHIFTS = (9, 10, 11), (0, 1, 2, 3)


@pytest.mark.parametrize("nbit", NBITS)
@pytest.mark.parametrize("s", SHIFTS)
def test_edge_words_by_brute_force(nbit, s):
    """each edge maps to its t, the word before the low edge and the word after the high edge fall into the neighbouring values
    (cyclically for abar; bbar's first and last intervals end at 0 and 2^32 - 1), consecutive intervals tile the 2^32 words, and the
    wrap -- a >= 2^32 - 2^(30 - nbit + s) -- gives abar = 0, never 2N"""
    E = es.edge_words(nbit, s)
    T, twoN, step = E.t.size, 2 << nbit, 1 << s
    assert T == twoN >> s and list(E.t[:3]) == [0, step, 2 * step] and E.t[-1] == twoN - step
    assert E.bbar[0] == twoN and E.bbar[-1] == step
    total_a = total_b = 0
    for i in range(T):
        t = int(E.t[i])
        alo, ahi, blo, bhi = int(E.a[i, 0]), int(E.a[i, 1]), int(E.b[i, 0]), int(E.b[i, 1])
        assert es.ms_abar(alo, nbit, s) == t and es.ms_abar(ahi, nbit, s) == t
        assert es.ms_abar((alo - 1) & es.M32, nbit, s) == (t - step) % twoN
        assert es.ms_abar((ahi + 1) & es.M32, nbit, s) == (t + step) % twoN
        total_a += ((ahi - alo) & es.M32) + 1
        bb = int(E.bbar[i])
        assert es.ms_bbar(blo, nbit, s) == bb and es.ms_bbar(bhi, nbit, s) == bb
        if i > 0:
            assert es.ms_bbar(blo - 1, nbit, s) == bb + step
        if i < T - 1:
            assert es.ms_bbar(bhi + 1, nbit, s) == bb - step
        total_b += bhi - blo + 1
    assert total_a == total_b == 1 << 32
    assert int(E.b[0, 0]) == 0 and int(E.b[-1, 1]) == es.M32
    half = 1 << (30 - nbit + s)
    assert int(E.a[0, 0]) == (1 << 32) - half and int(E.a[0, 1]) == half - 1
    for a in ((1 << 32) - half, es.M32, 0, half - 1):
        assert es.ms_abar(a, nbit, s) == 0
    assert es.ms_abar((1 << 32) - half - 1, nbit, s) == twoN - step


def _schoolbook_by_monomial(p, e, N, bits):
    """(X^e mod (X^N + 1)) * p, coefficient by coefficient in Python integers"""
    mono = [0] * N
    mono[e % N] = -1 if (e // N) & 1 else 1
    out = [0] * N
    for i in range(N):
        if mono[i]:
            for j in range(N):
                if i + j < N:
                    out[i + j] += mono[i] * int(p[j])
                else:
                    out[i + j - N] -= mono[i] * int(p[j])
    return np.array([v % (1 << bits) for v in out], dtype=es.DTYPE[bits])


@pytest.mark.parametrize("bits", [32, 64])
def test_rotate_is_multiplication_by_the_monomial(bits):
    N = 64
    rng = np.random.default_rng(2100 + bits)
    p = rng.integers(0, 1 << bits, N, dtype=np.uint64).astype(es.DTYPE[bits])
    p[[0, 1, N - 1]] = [0, (1 << (bits - 1)), (1 << bits) - 1]
    for e in range(2 * N + 1):
        want = _schoolbook_by_monomial(p, e, N, bits)
        assert np.array_equal(es.rotate(p, e), want), e
        assert np.array_equal(es.rotate_many(np.stack([p, p]), e, N), np.stack([want, want])), e


def test_every_exponent_against_the_existing_helpers(keys):
    """ms_* for both edge words of every exponent and rotate for every exponent: multi_output_checker, ps_user_gate_checker,
    lvl2_multi_checker, cb_checker, user_gate_checker, packed_rom_checker, lvl2_user_gate_checker, lut_checker (steps = 0)"""
    for nbit in NBITS:
        for s in SHIFTS:
            E = es.edge_words(nbit, s)
            for i in range(E.t.size):
                for a, b in zip(E.a[i], E.b[i]):
                    assert pc.ms_abar(a, s, nbit) == int(E.t[i]) == es.ms_abar(a, nbit, s)
                    assert pc.ms_bbar(b, s, nbit) == int(E.bbar[i]) == es.ms_bbar(b, nbit, s)
                    if nbit == 10:
                        assert mc.ms_abar(a, s) == int(E.t[i]) and mc.ms_bbar(b, s) == int(E.bbar[i])
                        if s == 0:
                            assert uc.mod_switch((int(a) + (1 << 20)) & es.M32) == int(E.t[i]) and 2 * ol.N - uc.mod_switch(b) == int(E.bbar[i])
                    if nbit == 11:
                        assert m2.ms_abar(a, s) == int(E.t[i]) and m2.ms_bbar(b, s) == int(E.bbar[i])
                        if s == 0:
                            assert cb._mod_switch((int(a) + (1 << 19)) & es.M32) == int(E.t[i]) and 2 * ol.N2 - cb._mod_switch(b) == int(E.bbar[i])
    rng = np.random.default_rng(2200)
    N, N2 = ol.N, ol.N2
    c = rng.integers(0, 1 << 32, 2 * N, dtype=np.uint64).astype(np.uint32)
    tv2 = rng.integers(0, 1 << 64, N2, dtype=np.uint64)
    x = rng.integers(0, 1 << 32, ol.n + 1, dtype=np.uint64).astype(np.uint32)
    for e in range(2 * N + 1):
        mine = np.concatenate([es.rotate(c[:N], e), es.rotate(c[N:], e)])
        assert np.array_equal(mine, np.concatenate([uc.negacyclic_rotate(c[:N], e), uc.negacyclic_rotate(c[N:], e)])), e
        assert np.array_equal(mine, es.rotate_many(c.reshape(2, N), e, N).reshape(-1)), e
        if e < 2 * N:
            assert np.array_equal(mine, pr.rotate(c, e)), e
        for Ns in (512, 1024):
            assert np.array_equal(es.rotate(c[:Ns], e % (2 * Ns)), pc.negacyclic_rotate(c[:Ns], e % (2 * Ns))), (Ns, e)
    for e in range(1, 2 * N2 + 1):
        assert np.array_equal(es.rotate(tv2, e), l2.rotated_tv(tv2, e)), e
        assert np.array_equal(es.rotate_many(tv2, e, N2), l2.rotated_tv(tv2, e)), e
    E = es.edge_words(10, 0)
    for s in SHIFTS:
        Es = es.edge_words(10, s)
        for i in range(Es.t.size):
            x[ol.n] = Es.b[i, i & 1]
            assert np.array_equal(es.start_acc("table", x[ol.n], s, 10, table=c), lc.lut_rotate(keys, x, c, s, steps=0)), (s, i)
    assert E.t.size == 2 * N


def test_extract_against_the_existing_helpers():
    rng = np.random.default_rng(2300)
    N, N2 = ol.N, ol.N2
    c = rng.integers(0, 1 << 32, 2 * N, dtype=np.uint64).astype(np.uint32)
    c2 = rng.integers(0, 1 << 64, 2 * N2, dtype=np.uint64)
    c3 = rng.integers(0, 1 << 32, 3 * 512, dtype=np.uint64).astype(np.uint32)
    for j in list(range(0, N, 37)) + [1, 63, 64, N - 1]:
        want = es.extract(c, j, N)
        assert np.array_equal(want, mc.sample_extract(c, j)) and np.array_equal(want, pr.extract_formula(c, j)), j
    for j in (0, 1, 7, 64, N2 - 1):
        assert np.array_equal(es.extract(c2, j, N2), m2.sample_extract(c2, j)), j
    chk = pc.Checker.__new__(pc.Checker)
    chk.N, chk.k = 512, 2
    for j in (0, 1, 7, 511):
        assert np.array_equal(es.extract(c3, j, 512, k=2), chk.sample_extract(c3, j)), j


def _sweep_b(nbit, n, seed):
    E = es.edge_words(nbit, 0)
    return E, es.sweep_rows(E, "b", n, np.random.default_rng(seed))


def test_start_acc_is_the_oracles_first_accumulator(keys, oracle):
    """orc_blind_rotate(steps = 0) and orc2_blind_rotate(steps = 0) at both edge words of every bbar"""
    E, rows = _sweep_b(10, ol.n, 2400)
    for g in range(rows.shape[0]):
        assert np.array_equal(es.start_acc("mu", rows[g, ol.n], 0, 10), keys.blind_rotate(rows[g], steps=0)), g
    keys2 = ol.KeysLvl2(oracle, keys, seed=7)
    E, rows = _sweep_b(11, ol.n, 2401)
    for g in range(rows.shape[0]):
        want = keys2.blind_rotate(rows[g], steps=0)
        assert np.array_equal(es.start_acc("mu", rows[g, ol.n], 0, 11, bits=64), want), g
        assert np.array_equal(es.start_acc("const", rows[g, ol.n], 0, 11, bits=64, const=ol.MU2), want), g


@pytest.mark.parametrize("name", ol.SETS)
def test_start_acc_on_the_parameter_sets(name):
    """the per-set oracle's first accumulator (k zero mask polynomials) at both edges of every bbar, and the set checker's with a
    random row under every shift"""
    C = pc.Checker(name, seed=5)
    E, rows = _sweep_b(C.nbit, C.n, 2500)
    for g in range(rows.shape[0]):
        assert np.array_equal(es.start_acc("mu", rows[g, C.n], 0, C.nbit, k=C.k), C.K.blind_rotate(rows[g], steps=0)), (name, g)
    tv = np.random.default_rng(2501).integers(0, 1 << 32, C.N, dtype=np.uint64).astype(np.uint32)
    for s in SHIFTS:
        Es = es.edge_words(C.nbit, s)
        rows = es.sweep_rows(Es, "b", C.n, np.random.default_rng(2502 + s))
        for g in range(0, rows.shape[0], 3):
            assert np.array_equal(es.start_acc("tv", rows[g, C.n], s, C.nbit, k=C.k, tv=tv), C.rotate(rows[g], tv, s, steps=0)), (name, s, g)
