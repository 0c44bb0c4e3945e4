"""CPU tests of the encrypted-table lookup: the checker tests/lut_checker.py on a trivial table (0, TV) is
the multi-output checker word for word; its `spread` makes the library's test vectors out of one value per box; pack + spread +
lookup IS a lookup, by decryption under genuine keys within the noise bound section 13 derives; the library exports the entry points
and refuses what needs no device work."""
import ctypes
import os

import numpy as np
import pytest

import lut_checker as lc
import multi_output_checker as mc
import oracle_lib as ol
import pack_checker as pk

n, N = ol.n, ol.N
NEW_SYMBOLS = ("cufhe_amd_lut_rotate_batch", "cufhe_amd_lut_lookup_batch", "cufhe_amd_trlwe_spread_batch")


def test_library_exports_the_new_entry_points():
    import cufhe_amd._lib as _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ol.ROOT, "include", "cufhe_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    import cufhe_amd.api as api
    for name in ("lut_rotate_batch", "lut_lookup_batch", "trlwe_spread_batch", "gLookupTRLWE", "gBlindRotateTRLWE", "gSpreadTRLWE"):
        assert callable(getattr(api, name))


@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_trivial_table_is_the_multi_output_checker(keys, s):
    """(0, TV) as the table: the accumulator of multi_output_checker.blind_rotate_tv_multi, every word"""
    rng = np.random.default_rng(1300 + s)
    tv = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
    x = rng.integers(0, 1 << 32, size=n + 1, dtype=np.uint64).astype(np.uint32)
    table = np.concatenate([np.zeros(N, np.uint32), tv])
    assert np.array_equal(lc.lut_rotate(keys, x, table, s), mc.blind_rotate_tv_multi(keys, x, tv, s))
    if s == 1:      # and the lookup is the level-0 multi-output gate with coefficients (1, 0, 0), offset 0
        want = mc.multi_gate_one(keys, 0, (1, 0, 0), 0, tv, 2, [x])
        assert np.array_equal(lc.lut_lookup(keys, x, table, 2), np.stack(want))


@pytest.mark.parametrize("nout", [1, 2, 8])
@pytest.mark.parametrize("p", [2, 4, 64])
def test_spread_makes_the_test_vectors(p, nout):
    """values[j][m] at coefficient m N / p + j, stride = nout, reps = N / (p nout): the numpy restatements and the library's own host
    builders, word for word -- the top half box holding -values[j][0] included.  The a polynomial carries other words through the same sum."""
    import cufhe_amd.api as api
    rng = np.random.default_rng(1400 + 10 * p + nout)
    values = rng.integers(0, 1 << 32, size=(nout, p), dtype=np.uint64).astype(np.uint32)
    c = np.zeros((2, N), np.uint32)
    for j in range(nout):
        c[1, np.arange(p) * (N // p) + j] = values[j]
    c[0] = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
    got = lc.spread(c, nout, N // (p * nout)).reshape(2, N)
    assert np.array_equal(got[1], mc.test_vector_multi(values))
    assert np.array_equal(got[1], api.test_vector_multi(values) if nout > 1 else api.test_vector(values[0]))
    if nout == 1:
        assert np.array_equal(got[1], lc.test_vector(values[0]))
    # the a polynomial went through the same sum: compare it with the sum written out at three coefficients
    reps, stride = N // (p * nout), nout
    for k in (0, N // 2 + 1, N - 1):
        want = 0
        for i in range(reps):
            idx = k + stride * (reps // 2) - i * stride
            want += (-1) ** (idx // N) * int(c[0, idx % N])
        assert int(got[0, k]) == want % (1 << 32)


def lookup_sigma(entry_variance):
    """section 13: the table's error at the addressed coefficient + the blind rotation + the key switch, torus units.  A table made by
    pack + Spread carries, at every coefficient, the addressed entry's own error and packing rounding ((n / 2) 2^-34 / 3) plus the pack
    key's noise: `reps` coefficients of the packed TRLWE summed, each holding n t rows of sigma 2^-25 for each of the p inputs of that
    TRLWE -- reps p = N whatever p is."""
    a0, a1 = 2.0 ** -15, 2.0 ** -25
    rotation = n * (2 * 3 * N * 64.0 ** 2 / 12 * a1 ** 2 + (1 + N / 2) * (2.0 ** -19) ** 2 / 3)
    keyswitch = N * 8 * 0.75 * a0 ** 2 + (N / 2) * (2.0 ** -17) ** 2 / 3
    table = entry_variance + (n / 2) * 2.0 ** -34 / 3 + N * n * pk.T * pk.KEY_SIGMA ** 2
    return np.sqrt(table + rotation + keyswitch), rotation, keyswitch


@pytest.fixture(scope="module")
def pack_key(keys):
    return pk.genuine_key(keys, seed=1501)


@pytest.mark.parametrize("p", [4, 8])
def test_it_is_a_lookup_under_genuine_keys(keys, pack_key, p):
    """p host-encrypted entries (values of the padded p-ary encoding, sigma = alpha0 = 2^-15) packed at m N / p by the checker's
    pack_batch, spread over their boxes, then read by a host-encrypted address m 2^32 / (2p) for every m: the phase of output 0 minus
    the entry's value is within six sigma of the bound derived from the parameters (lookup_sigma), and the address picks entry m."""
    import user_gate_checker as uc
    rng = np.random.default_rng(1500 + p)
    alpha0 = 2.0 ** -15
    sigma, rotation, keyswitch = lookup_sigma(alpha0 ** 2)
    assert abs(rotation - 1.57e-6) < 0.01e-6 and abs(keyswitch - 5.73e-6) < 0.01e-6        # the figures INTEGRATION.md quotes
    assert 0.0026 < sigma < 0.0028
    step = (1 << 32) // (2 * p)
    msgs = rng.permutation(p).astype(np.uint64) * np.uint64(step)      # a permutation: every entry differs from every other
    entries = uc.encrypt_torus(keys, 0, msgs, alpha0 * 2.0 ** 32, seed=1510 + p)
    pos = (np.arange(p) * (N // p)).astype(np.int32)
    packed = pk.pack_batch(pack_key, entries, np.zeros(p, np.int32), pos, 1)[0]
    table = lc.spread(packed, 1, N // p)
    addr = uc.encrypt_torus(keys, 0, np.arange(p, dtype=np.uint64) * np.uint64(step), alpha0 * 2.0 ** 32, seed=1520 + p)
    outs = lc.on_threads(lambda m: lc.lut_lookup(keys, addr[m], table, 1)[0], p)
    err = pk.signed(uc.phase(keys, 0, np.stack(outs)).astype(np.int64) - msgs.astype(np.int64)) / 2.0 ** 32
    print(f"p = {p}: max |phase - entry| {np.abs(err).max():.3e} of the torus, sigma {sigma:.3e}, bound {6 * sigma:.3e}")
    assert np.abs(err).max() < 6 * sigma, (err, sigma)
    assert 6 * sigma < 1.0 / (4 * p)      # and that is inside half a box: the nearest entry is the addressed one


def test_refusals_that_need_no_device_work():
    import cufhe_amd._lib as _lib
    lib = _lib.lib
    fake, fake2 = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 28)      # never dereferenced: every call is refused before any device work
    ok = np.zeros(3, np.int32)

    def refused(rc, *words):
        msg = lib.cufhe_amd_last_error()
        assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)

    for fn, extra in ((lib.cufhe_amd_lut_rotate_batch, (-1,)), (lib.cufhe_amd_lut_lookup_batch, ())):
        def call(tlwe0=fake, tables=fake2, table_count=2, src=ok.ctypes.data, nout=1, out=ctypes.c_void_p(1 << 30), count=3):
            return fn(0, None, count, tlwe0, tables, table_count, src, nout, *extra, out)
        refused(call(tlwe0=None), b"null")
        refused(call(tables=None), b"null")
        refused(call(out=None), b"null")
        for bad in (0, 3, 5, 16, -1):
            refused(call(nout=bad), b"nout")
        for bad in (-1, 2):
            s = ok.copy()
            s[1] = bad
            refused(call(src=s.ctypes.data), b"src")
        refused(call(src=None), b"src")                       # src NULL means src[g] = g: 3 rotations need 3 tables
        refused(call(table_count=0), b"table_count")
        refused(call(out=ctypes.c_void_p((1 << 28) + 4 * (2 * N + 5))), b"overlap")       # inside table 1
        refused(call(out=ctypes.c_void_p((1 << 28) - 8)), b"overlap")                     # runs into table 0
    sp = lib.cufhe_amd_trlwe_spread_batch
    refused(sp(0, None, 2, None, 1, 1, fake2), b"null")
    refused(sp(0, None, 2, fake, 1, 1, None), b"null")
    for stride, reps in ((0, 1), (-1, 4), (1, 0), (4, -1), (1, N + 1), (N + 1, 1), (3, 342), (1 << 20, 1 << 20)):
        refused(sp(0, None, 2, fake, stride, reps, fake2), b"stride")
    refused(sp(0, None, 2, fake, 1, 4, fake), b"overlap")
    refused(sp(0, None, 2, fake, 1, 4, ctypes.c_void_p((1 << 20) + 4 * (4 * N - 1))), b"overlap")
    # (well-formed arguments without keys, -3, and "param_set": tests/test_gpu_lut.py, with real device buffers)


def test_cpp_program_compiles():
    """tests/cpp/test_lut.cpp builds against include/cufhe_amd.hpp, the library and the oracle (it runs in the GPU suite)"""
    assert os.path.exists(lc.build_cpp_program())
