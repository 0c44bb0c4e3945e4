"""GPU tests of the encrypted-table lookup.  Word parity is equality of every word with
tests/lut_checker.py on random words (parity needs no valid ciphertext), on every blind-rotate kernel and across the segments of
one launch; tables (0, TV) give the words of the user gates on TV; one end-to-end case under genuine keys is the worked example of
section 13 -- gates, packing, Spread, lookup -- with zero decrypt errors.  The C++ mirror tests/cpp/test_lut.cpp and the refusals
run last."""
import subprocess

import numpy as np
import pytest

import lut_checker as lc
import multi_output_checker as mc
import oracle_lib as ol
import pack_checker as pk
import user_gate_checker as uc
from test_gpu_user_gates import run_batch, set_shape, up

pytestmark = pytest.mark.gpu

N, n = ol.N, ol.n
MU = ol.MU
FILL = 0xA5A5A5A5
SHAPES = ["batch", "half", "ll", "ll2"]
NOUTS = [1, 2, 4, 8]
TABLES, PAIRS, ROTATIONS = 5, 7, 19
FULL_NOUT = {"batch": 1, "half": 2, "ll": 4, "ll2": 8}       # the nout of the three full-length rotations of a shape


def reinit(engine, keys):
    engine.CleanUp()
    engine.SetGPUNum(1)
    engine.Initialize(keys.bk, keys.ksk)


@pytest.fixture
def fresh(engine, keys):
    """a freshly initialised engine before and after: no user gates, no packing key left behind for the files that follow"""
    reinit(engine, keys)
    yield engine
    reinit(engine, keys)


class Data:
    """5 tables and 7 lvl0 ciphertexts of random words, 7 distinct (table, ciphertext) pairs, and the checker's accumulators of the
    pairs: computed once per (nout, steps) and shared by the tests"""

    def __init__(self, keys):
        rng = np.random.default_rng(1600)
        self.keys = keys
        self.tables = rng.integers(0, 1 << 32, size=(TABLES, 2 * N), dtype=np.uint64).astype(np.uint32)
        self.x = rng.integers(0, 1 << 32, size=(PAIRS, n + 1), dtype=np.uint64).astype(np.uint32)
        self.x[0, n] = 0                                       # bbar = 2N: the unrotated table
        self.x[1, n] = 0xFFFFFFFF                              # bbar = 1 at nout = 1
        self.pair_table = np.array([g % TABLES for g in range(PAIRS)], np.int32)
        self._acc = {}

    def acc(self, nout, steps, pairs=range(PAIRS)):
        s = mc.shift_of(nout)
        todo = [q for q in pairs if (q, nout, steps) not in self._acc]
        got = lc.on_threads(lambda i: lc.lut_rotate(self.keys, self.x[todo[i]], self.tables[self.pair_table[todo[i]]], s, steps), len(todo))
        for q, a in zip(todo, got):
            self._acc[(q, nout, steps)] = a
        return np.stack([self._acc[(q, nout, steps)] for q in pairs])


@pytest.fixture(scope="module")
def data(keys):
    return Data(keys)


def rotate(engine, x, tables, src, nout, steps, table_count=None):
    count = x.shape[0]
    dx, dt = up(engine, x), up(engine, tables)
    dacc = up(engine, np.full(count * 2 * N, FILL, np.uint32))
    engine.api.lut_rotate_batch(dx, dt, dacc, count, tables.shape[0] if table_count is None else table_count, src=src, nout=nout, steps=steps)
    engine.Synchronize()
    return dacc.download().reshape(count, 2 * N)


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "%d words differ, first at (rotation, word) %s" % (len(bad), tuple(bad[0]) if len(bad) else None)


@pytest.mark.parametrize("shape", SHAPES)
def test_rotation_words_on_every_kernel(engine, data, shape):
    """19 rotations tiled from the 7 pairs -- three workgroups of 8 with idle waves in the last, five of 4, an odd count for the paired
    kernel -- with src repeating tables, for nout 1, 2, 4, 8 at 3 steps; src NULL (rotation g reads table g); and three full-length
    rotations: every word of every accumulator equals the checker's"""
    api = engine.api
    pair = np.arange(ROTATIONS) % PAIRS
    src = data.pair_table[pair]
    assert len(set(src)) == TABLES and len(src) > len(set(src))
    set_shape(api, shape)
    try:
        for nout in NOUTS:
            want = data.acc(nout, 3)[pair]
            got = rotate(engine, data.x[pair], data.tables, src, nout, 3)
            assert np.array_equal(got, want), (shape, nout, first_difference(got, want))
        # src NULL: rotation g names table g, so pairs 0 .. 4 as they are (pair q reads table q there)
        got = rotate(engine, data.x[:TABLES], data.tables, None, 2, 3)
        want = data.acc(2, 3)[:TABLES]
        assert np.array_equal(got, want), (shape, "src NULL", first_difference(got, want))
        # all n steps (steps outside [0, n] means n)
        nout = FULL_NOUT[shape]
        want = data.acc(nout, n, range(3))
        got = rotate(engine, data.x[:3], data.tables, data.pair_table[:3], nout, -1)
        assert np.array_equal(got, want), (shape, "n steps", first_difference(got, want))
        got = rotate(engine, data.x[:3], data.tables, data.pair_table[:3], nout, n + 1)
        assert np.array_equal(got, want), (shape, "steps > n", first_difference(got, want))
    finally:
        set_shape(api, None)


def test_every_segment_reads_its_own_tables(engine, data):
    """8 cus + 5 rotations under the default rules: one full round of the batch kernel and a tail segment on another kernel.  Every
    row of acc equals its reference: a table-pointer array that is not offset by the segment's first rotation would give the tail
    the tables of rotations 0 .. 4"""
    count = 8 * engine.api.device_cus() + 5
    pair = (np.arange(count) * 3 + 1) % PAIRS                  # the tail's pairs differ from those of rotations 0 .. 4
    assert not np.array_equal(pair[:5], pair[-5:])
    want = data.acc(1, 3)[pair]
    got = rotate(engine, data.x[pair], data.tables, data.pair_table[pair], 1, 3)
    assert np.array_equal(got, want), first_difference(got, want)


@pytest.mark.parametrize("nout", [1, 4])
def test_trivial_tables_give_the_user_gates_words(fresh, keys, nout):
    """tables (0, TV): lut_lookup_batch returns the words gate_batch returns for a user gate (nout = 4: every output of the
    multi-output definition) with coefficients (1, 0, 0) and offset 0 on the same TV"""
    eng, api = fresh, fresh.api
    rng = np.random.default_rng(1700 + nout)
    count = 6
    tv = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
    x = rng.integers(0, 1 << 32, size=(count, n + 1), dtype=np.uint64).astype(np.uint32)
    op = api.define_gate((1, 0, 0), 0, tv, nout=nout)
    want = np.stack([run_batch(eng, api.user_op_output(op, j) if nout > 1 else op, 0, [x], count) for j in range(nout)], axis=1)
    table = np.concatenate([np.zeros(N, np.uint32), tv])
    dx, dt, dout = up(eng, x), up(eng, table), up(eng, np.full(count * nout * (n + 1), FILL, np.uint32))
    api.lut_lookup_batch(dx, dt, dout, count, 1, src=np.zeros(count, np.int32), nout=nout)
    eng.Synchronize()
    got = dout.download().reshape(count, nout, n + 1)
    assert np.array_equal(got, want), first_difference(got.reshape(count, -1), want.reshape(count, -1))


@pytest.mark.parametrize("nout", [1, 2, 8])
def test_lookup_words(engine, data, nout):
    """5 items on the default shape: all nout outputs of every item equal the checker's key switch of SampleExtract(j)"""
    api = engine.api
    count = 5
    pair = np.array([0, 3, 6, 3, 1])
    acc = data.acc(nout, n, sorted(set(pair)))
    by_pair = dict(zip(sorted(set(pair)), acc))
    want = np.stack([np.stack([data.keys.keyswitch(mc.sample_extract(by_pair[q], j)) for j in range(nout)]) for q in pair])
    dx, dt = up(engine, data.x[pair]), up(engine, data.tables)
    dout = up(engine, np.full(count * nout * (n + 1), FILL, np.uint32))
    api.lut_lookup_batch(dx, dt, dout, count, TABLES, src=data.pair_table[pair], nout=nout)
    engine.Synchronize()
    got = dout.download().reshape(count, nout, n + 1)
    assert np.array_equal(got, want), first_difference(got.reshape(count, -1), want.reshape(count, -1))
    assert np.array_equal(dt.download().reshape(TABLES, -1), data.tables)


SPREADS = [(1, 1), (1, 2), (1, 3), (1, 256), (1, 1024), (4, 64), (8, 128), (3, 341)]
_spread_ref = {}


def spread_reference(stride, reps):
    """5 random TRLWEs and the checker's Spread of each, once per (stride, reps)"""
    if (stride, reps) not in _spread_ref:
        c = np.random.default_rng(1800).integers(0, 1 << 32, size=(5, 2 * N), dtype=np.uint64).astype(np.uint32)
        _spread_ref[(stride, reps)] = (c, np.stack([lc.spread(c[g], stride, reps) for g in range(5)]))
    return _spread_ref[(stride, reps)]


@pytest.mark.parametrize("count", [1, 5, 65])
@pytest.mark.parametrize("stride,reps", SPREADS)
def test_spread_words(engine, stride, reps, count):
    """every word of every polynomial: 65 TRLWEs (tiled from the five) are 33 workgroups, the last with two idle waves"""
    c, want = spread_reference(stride, reps)
    item = np.arange(count) % 5
    din, dout = up(engine, c[item]), up(engine, np.full(count * 2 * N, FILL, np.uint32))
    engine.api.trlwe_spread_batch(din, dout, count, stride, reps)
    engine.Synchronize()
    got = dout.download().reshape(count, 2 * N)
    assert np.array_equal(got, want[item]), (stride, reps, first_difference(got, want[item]))
    assert np.array_equal(din.download().reshape(count, -1), c[item])


@pytest.fixture(scope="module")
def pack_key_words(keys):
    return pk.genuine_key(keys, seed=1901)


def test_worked_example_end_to_end(fresh, keys, pack_key_words):
    """Section 13's example through the object forms, p = 4: four Xor gates make the entries, gPackTLWEs puts entry m at m N / 4,
    gSpreadTRLWE fills the boxes, gLookupTRLWE reads by the padded address m / 8.  Every address, both values of every entry (two
    tables, one the complement of the other), addresses host-encrypted at the oracle's lvl0 sigma; and once the address is made on
    the device by a one-input user gate.  Zero decrypt errors: section 13 derives more than 15 sigma for p = 4."""
    eng, api = fresh, fresh.api
    api.pack_initialize(pack_key_words)
    st = api.Stream()
    st.Create()
    rng = np.random.default_rng(1900)
    a = rng.integers(0, 2, size=4).astype(np.uint8)
    errors = 0
    for flip in (0, 1):
        b = a ^ np.array([0, 1, 1, 0], np.uint8) ^ flip                  # v = a ^ b = 0 1 1 0, then 1 0 0 1
        v = a ^ b
        ea, eb = keys.encrypt(a, 0, seed=1910 + flip), keys.encrypt(b, 0, seed=1920 + flip)
        ca, cb, cv = [api.Ctxt(0) for _ in range(4)], [api.Ctxt(0) for _ in range(4)], [api.Ctxt(0) for _ in range(4)]
        for m in range(4):
            ca[m].tlwehost[:] = ea[m]
            cb[m].tlwehost[:] = eb[m]
            api.Xor(cv[m], ca[m], cb[m], st)                             # table entries made by gates
        packed, table = api.Trlwe(), api.Trlwe()
        api.gPackTLWEs(packed, cv, [m * N // 4 for m in range(4)], st)   # entry m at coefficient m N / p
        api.gSpreadTRLWE(table, packed, 1, N // 4, st)                   # boxes, the top half box = -v[0]
        addrs = uc.encrypt_torus(keys, 0, np.arange(4, dtype=np.uint64) * np.uint64(MU), 2.0 ** 17, seed=1930 + flip)
        for m in range(4):
            addr, out = api.Ctxt(0), api.Ctxt(0)
            addr.tlwehost[:] = addrs[m]
            api.CtxtCopyH2D(addr, st)
            api.gLookupTRLWE([out], table, addr, st)                     # addr: the padded message m / 8
            api.CtxtCopyD2H(out, st)
            api.Synchronize()
            got = int(keys.decrypt(out.tlwehost, 0)[0])
            errors += got != int(v[m])
            assert got == int(v[m]), (flip, m, got, list(v))
        if flip == 0:
            # the address made on the device: a +-1/8 bit through x = in + 1/8 and TestVector({0, 0, 1/8, 1/8}) is the padded message
            # 0 or 1, so it reads entry 0 or entry 1
            to_msg = api.define_gate((1, 0, 0), MU, api.test_vector(np.array([0, 0, MU, MU], np.uint32)))
            ebit = keys.encrypt(np.array([0, 1], np.uint8), 0, seed=1940)
            for bit in (0, 1):
                cbit, addr, out = api.Ctxt(0), api.Ctxt(0), api.Ctxt(0)
                cbit.tlwehost[:] = ebit[bit]
                api.Apply(to_msg, addr, cbit, st)                        # recorded: launched by the fence inside gLookupTRLWE
                api.gLookupTRLWE([out], table, addr, st)
                api.CtxtCopyD2H(out, st)
                api.Synchronize()
                assert int(keys.decrypt(out.tlwehost, 0)[0]) == int(v[bit]), (bit, list(v))
        # the table itself: the words of the checker's Spread of the packed TRLWE, and the rotation alone extracts the same entry
        api.CtxtCopyD2H(packed, st)
        api.CtxtCopyD2H(table, st)
        api.Synchronize()
        assert np.array_equal(table.trlwehost, lc.spread(packed.trlwehost, 1, N // 4))
    assert errors == 0
    addr, rot, out = api.Ctxt(0), api.Trlwe(), api.Ctxt(0)
    addr.tlwehost[:] = addrs[2]
    api.CtxtCopyH2D(addr, st)
    api.gBlindRotateTRLWE(rot, table, addr, st)
    api.gSampleExtractAndKeySwitch(out, rot, st, index=0)
    api.CtxtCopyD2H(out, st)
    api.Synchronize()
    assert int(keys.decrypt(out.tlwehost, 0)[0]) == int(v[2])
    st.Destroy()


def test_refusals_and_the_ops_around_them(engine, keys, data):
    """every row of the refusal table of section 13 with real device buffers, each before any device work (the outputs keep their
    fill); Spread runs without keys; a valid call afterwards succeeds and a NAND batch in the same session gives the oracle's words"""
    api, lib = engine.api, engine.lib
    count = 3
    ok = np.zeros(count, np.int32)
    dx, dt = up(engine, data.x[:count]), up(engine, data.tables)
    dacc = up(engine, np.full(count * 2 * N, FILL, np.uint32))
    dout = up(engine, np.full(count * 8 * (n + 1), FILL, np.uint32))

    def rot(tlwe0=dx.ptr, tables=dt.ptr, table_count=TABLES, src=ok.ctypes.data, nout=1, acc=dacc.ptr, c=count):
        return lib.cufhe_amd_lut_rotate_batch(0, None, c, tlwe0, tables, table_count, src, nout, 3, acc)

    def look(tlwe0=dx.ptr, tables=dt.ptr, table_count=TABLES, src=ok.ctypes.data, nout=1, out=dout.ptr, c=count):
        return lib.cufhe_amd_lut_lookup_batch(0, None, c, tlwe0, tables, table_count, src, nout, out)

    def refused(rc, word):
        assert rc == -1 and word in lib.cufhe_amd_last_error(), (rc, lib.cufhe_amd_last_error())

    for call, outname in ((rot, "acc"), (look, "out")):
        refused(call(tlwe0=None), b"null")
        refused(call(tables=None), b"null")
        refused(call(**{outname: None}), b"null")
        for bad in (0, 3, 16):
            refused(call(nout=bad), b"nout")
        for bad in (-1, TABLES):
            s = ok.copy()
            s[2] = bad
            refused(call(src=s.ctypes.data), b"src")
        refused(call(table_count=0), b"table_count")
        refused(call(src=None, table_count=2), b"src")                   # src NULL: rotation 2 would read table 2 of 2
        refused(call(**{outname: dt.ptr + 4 * (2 * N + 7)}), b"overlap")
    sp = lib.cufhe_amd_trlwe_spread_batch
    refused(sp(0, None, count, None, 1, 4, dacc.ptr), b"null")
    refused(sp(0, None, count, dt.ptr, 1, 4, None), b"null")
    for stride, reps in ((0, 4), (1, 0), (-2, 4), (2, 513), (1, N + 1)):
        refused(sp(0, None, count, dt.ptr, stride, reps, dacc.ptr), b"stride")
    refused(sp(0, None, count, dt.ptr, 1, 4, dt.ptr), b"overlap")
    refused(sp(0, None, count, dt.ptr, 1, 4, dt.ptr + 4 * (3 * 2 * N - 1)), b"overlap")
    ps = api.ps_index("default")
    api.ps_initialize(ps, keys.bk, keys.ksk)
    api.set_option("param_set", ps)
    try:
        for rc in (rot(), look(), sp(0, None, count, dt.ptr, 1, 4, dacc.ptr)):
            assert rc == -1 and b"param_set" in lib.cufhe_amd_last_error() and b"default path only" in lib.cufhe_amd_last_error()
    finally:
        api.set_option("param_set", -1)
    # without keys: the rotations are refused with -3, Spread needs none
    engine.CleanUp()
    engine.SetGPUNum(1)
    try:
        assert rot() == -3 and b"Initialize" in lib.cufhe_amd_last_error()
        assert look() == -3 and b"Initialize" in lib.cufhe_amd_last_error()
        engine.Synchronize()
        assert np.all(dacc.download() == FILL) and np.all(dout.download() == FILL) and np.array_equal(dt.download().reshape(TABLES, -1), data.tables)
        api.trlwe_spread_batch(dt, dacc, count, 4, 64)
        engine.Synchronize()
        want = np.stack([lc.spread(data.tables[g], 4, 64) for g in range(count)])
        assert np.array_equal(dacc.download().reshape(count, -1), want)
    finally:
        engine.Initialize(keys.bk, keys.ksk)
    # a following valid call succeeds, and the built-in gates are what they were
    pair = np.arange(count)
    got = rotate(engine, data.x[pair], data.tables, data.pair_table[pair], 1, 3)
    assert np.array_equal(got, data.acc(1, 3)[pair])
    bits = np.random.default_rng(1950).integers(0, 2, size=(2, 16)).astype(np.uint8)
    a, b = keys.encrypt(bits[0], 0, seed=1951), keys.encrypt(bits[1], 0, seed=1952)
    assert np.array_equal(run_batch(engine, api.NAND, 0, [a, b], 16), keys.gate_batch(api.NAND, 0, a, b))


def test_cpp_lut(engine, keys):
    """tests/cpp/test_lut.cpp: the worked example through include/cufhe_amd.hpp"""
    exe = lc.build_cpp_program()
    engine.CleanUp()                      # the C++ program owns the device state while it runs
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        engine.SetGPUNum(1)
        engine.Initialize(keys.bk, keys.ksk)
