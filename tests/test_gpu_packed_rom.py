"""GPU tests of the packed-ROM operations: TRLWE rotation by X^e, the rotating CMUX, SampleExtract at a
caller's index with and without the key switch, their recorded forms and the C++ mirror.  Everything is integer arithmetic: every
comparison is equality of every output word at every batch position against tests/packed_rom_checker.py, no tolerance."""
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import packed_rom_checker as pr

pytestmark = pytest.mark.gpu

N, n = ol.N, ol.n
TRGSW_WORDS = 12 * N                  # (k+1) l rows of k+1 polynomials; as many doubles in the NTT domain
COUNTS = [1, 5, 67]                   # one wave; more than one block of 4 waves with a partial one; many blocks and an odd tail
FILL = 0xA5A5A5A5


def up(eng, arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    return eng.api.DeviceBuffer(arr.size).upload(arr)


def random_trlwes(rng, count):
    return rng.integers(0, 1 << 32, size=(count, 2 * N), dtype=np.uint64).astype(np.uint32)


def exponents(rng, count):
    e = [pr.EXPONENTS[g % len(pr.EXPONENTS)] for g in range(count)]
    for g in range(len(pr.EXPONENTS), count, 2):          # every second one past the first cycle: random
        e[g] = int(rng.integers(0, 2 * N))
    return np.array(e, np.int32)


def to_ntt(eng, trgsw, copies=1):
    """the NTT image of one torus-domain TRGSW, `copies` times in a row (cufhe_amd_cmux_batch takes one TRGSW per item)"""
    d = up(eng, np.tile(np.ascontiguousarray(trgsw, np.uint32).ravel(), copies))
    dntt = eng.api.DeviceBuffer(copies * TRGSW_WORDS * 2)
    eng.api.trgsw_to_ntt_batch(d, dntt, copies)
    return dntt


@pytest.fixture(scope="module")
def selectors(keys):
    """a TRGSW of bit 1 and one of bit 0 under the lvl1 key (steps of the oracle's bootstrapping key)"""
    return {1: pr.selector(keys, 1), 0: pr.selector(keys, 0)}


@pytest.mark.parametrize("count", COUNTS)
def test_rotation(engine, count):
    api, lib = engine.api, engine.lib
    rng = np.random.default_rng(400 + count)
    c = random_trlwes(rng, count)
    e = exponents(rng, count)
    din, dout = up(engine, c), up(engine, np.full(count * 2 * N, FILL, np.uint32))
    api.trlwe_rotate_batch(din, e, dout, count)
    engine.Synchronize()
    got = dout.download().reshape(count, -1)
    want = np.stack([pr.rotate(c[g], int(e[g])) for g in range(count)])
    assert np.array_equal(got, want)
    # an exponent outside [0, 2N): refused, out untouched
    for bad in (-1, 2 * N):
        eb = e.copy()
        eb[count - 1] = bad
        assert lib.cufhe_amd_trlwe_rotate_batch(0, None, count, din.ptr, eb.ctypes.data, dout.ptr) == -1
    engine.Synchronize()
    assert np.array_equal(dout.download().reshape(count, -1), want)


@pytest.mark.parametrize("count", COUNTS)
def test_rotating_cmux(engine, oracle, selectors, count):
    api, lib = engine.api, engine.lib
    rng = np.random.default_rng(500 + count)
    c = random_trlwes(rng, count)
    e = exponents(rng, count)
    dc = up(engine, c)
    for bit in (1, 0):
        trgsw = selectors[bit]
        dntt, dntt_rep = to_ntt(engine, trgsw), to_ntt(engine, trgsw, count)
        want = np.stack([pr.cmux_rotate(oracle, trgsw, c[g], int(e[g])) for g in range(count)])
        # out of place
        dres = up(engine, np.full(count * 2 * N, FILL, np.uint32))
        api.cmux_rotate_batch(dntt, e, dc, dres, count)
        engine.Synchronize()
        assert np.array_equal(dres.download().reshape(count, -1), want), f"selector of bit {bit}, out of place"
        assert np.array_equal(dc.download().reshape(count, -1), c)
        # in place: res == c
        dinp = up(engine, c)
        api.cmux_rotate_batch(dntt, e, dinp, dinp, count)
        engine.Synchronize()
        assert np.array_equal(dinp.download().reshape(count, -1), want), f"selector of bit {bit}, in place"
        # the two-kernel sequence on the GPU: X^e c stored, then CMUXNTT with one copy of the selector per item
        drot, dseq = api.DeviceBuffer(count * 2 * N), api.DeviceBuffer(count * 2 * N)
        api.trlwe_rotate_batch(dc, e, drot, count)
        api.cmux_batch(dntt_rep, drot, dc, dseq, count)
        engine.Synchronize()
        assert np.array_equal(dseq.download().reshape(count, -1), want), f"selector of bit {bit}, rotate then CMUXNTT"
        # e = 0: c + trgsw [x] 0, the words of cmux_batch(trgsw, c, c)
        dzero, dsame = api.DeviceBuffer(count * 2 * N), api.DeviceBuffer(count * 2 * N)
        api.cmux_rotate_batch(dntt, np.zeros(count, np.int32), dc, dzero, count)
        api.cmux_batch(dntt_rep, dc, dc, dsame, count)
        engine.Synchronize()
        got0 = dzero.download().reshape(count, -1)
        assert np.array_equal(got0, dsame.download().reshape(count, -1))
        assert np.array_equal(got0[0], pr.cmux(oracle, trgsw, c[0], c[0]))
        # refused exponents: res untouched
        for bad in (-1, 2 * N):
            eb = e.copy()
            eb[0] = bad
            assert lib.cufhe_amd_cmux_rotate_batch(0, None, count, dntt.ptr, eb.ctypes.data, dc.ptr, dres.ptr) == -1
        engine.Synchronize()
        assert np.array_equal(dres.download().reshape(count, -1), want)


@pytest.mark.parametrize("with_src", [True, False])
def test_indexed_extraction(engine, keys, oracle, with_src):
    """67 outputs over 5 source TRLWEs (shared sources), or over 67 of their own with src = NULL"""
    api, lib = engine.api, engine.lib
    count = 67
    sources = 5 if with_src else count
    rng = np.random.default_rng(600 + with_src)
    c = random_trlwes(rng, sources)
    idx = np.array([pr.INDICES[g % len(pr.INDICES)] for g in range(count)], np.int32)
    src = np.array([(3 * g) % sources for g in range(count)], np.int32) if with_src else None
    of = (lambda g: int(src[g])) if with_src else (lambda g: g)
    dc = up(engine, c)
    d1 = up(engine, np.full(count * (N + 1), FILL, np.uint32))
    d0 = up(engine, np.full(count * (n + 1), FILL, np.uint32))
    api.sample_extract_index_batch(dc, idx, d1, count, src=src)
    api.sample_extract_index_keyswitch_batch(dc, idx, d0, count, src=src)
    engine.Synchronize()
    want1 = np.stack([pr.extract_by_rotation(oracle, c[of(g)], int(idx[g])) for g in range(count)])
    assert np.array_equal(want1, np.stack([pr.extract_formula(c[of(g)], int(idx[g])) for g in range(count)]))
    want0 = np.stack([keys.keyswitch(want1[g]) for g in range(count)])
    got1, got0 = d1.download().reshape(count, -1), d0.download().reshape(count, -1)
    assert np.array_equal(got1, want1)
    assert np.array_equal(got0, want0)
    # idx = 0 rows are the existing extraction at 0
    zero = np.flatnonzero(idx == 0)
    dz, dzo = up(engine, np.stack([c[of(g)] for g in zero])), api.DeviceBuffer(zero.size * (n + 1))
    api.sample_extract_keyswitch_batch(dz, dzo, zero.size)
    engine.Synchronize()
    assert np.array_equal(dzo.download().reshape(zero.size, -1), got0[zero])
    # refused indices: outputs untouched
    sp = src.ctypes.data if with_src else None
    for bad in (-1, N):
        ib = idx.copy()
        ib[count - 1] = bad
        assert lib.cufhe_amd_sample_extract_index_batch(0, None, count, dc.ptr, sp, ib.ctypes.data, d1.ptr) == -1
        assert lib.cufhe_amd_sample_extract_index_keyswitch_batch(0, None, count, dc.ptr, sp, ib.ctypes.data, d0.ptr) == -1
    engine.Synchronize()
    assert np.array_equal(d1.download().reshape(count, -1), want1) and np.array_equal(d0.download().reshape(count, -1), want0)


def test_recorded_rom_program(engine, keys):
    """2 TRLWEs x 4 words of 8 bits read at all 8 addresses: two in-place rotating CMUX steps on both TRLWEs, one CMUXNTT on the high
    bit, 8 indexed extractions with key switch -- recorded, one Synchronize.  Word for word the oracle composition, decrypting to the
    ROM word; CUFHE_AMD_TL_SEIKS_AT(0) gives the words of CUFHE_AMD_TL_SEIKS."""
    api, lib = engine.api, engine.lib
    table = pr.rom_table(700)
    trlwes = pr.rom_trlwes(keys, table, seed=701)
    st = api.Stream()
    st.Create()
    sel_words = {(k, bit): pr.selector(keys, bit, which=k) for k in range(3) for bit in (0, 1)}
    for addr in range(8):
        bits = [(addr >> k) & 1 for k in range(3)]
        words = [sel_words[(k, bits[k])] for k in range(3)]
        want = pr.rom_read(keys, trlwes, words)
        sels = [api.TrgswNtt() for _ in range(3)]
        for k in range(3):
            engine.check(lib.cufhe_amd_trgsw_to_ntt(st.device_id(), st.st(), words[k].ctypes.data, sels[k]._h))
        c = [api.Trlwe() for _ in range(2)]
        for t in range(2):
            c[t].trlwehost[:] = trlwes[t]
            api.CtxtCopyH2D(c[t], st)
        root = api.Trlwe()
        outs = [api.Ctxt(0) for _ in range(8)]
        old = api.Ctxt(0)
        for t in range(2):
            for k, e in enumerate(pr.ROM_EXPONENTS):
                api.gCMUXRotateNTT(c[t], sels[k], c[t], e, st)
        api.gCMUXNTT(root, sels[2], c[1], c[0], st)
        for b in range(8):
            api.gSampleExtractAndKeySwitch(outs[b], root, st, index=b)
            api.CtxtCopyD2H(outs[b], st)
        api._trlwe_op(api.TL_SEIKS, False, old, root, st)          # the existing op on the same device buffer
        api.CtxtCopyD2H(old, st)
        api.Synchronize()
        got = np.stack([o.tlwehost for o in outs])
        assert np.array_equal(got, want), f"address {addr}"
        word = sum(int(b) << i for i, b in enumerate(keys.decrypt(got, 0)))
        assert word == int(table[addr >> 2, addr & 3]), f"address {addr}"
        assert np.array_equal(old.tlwehost, got[0]), "SEIKS_AT(0) != SEIKS"
    st.Destroy()


def test_refusals(engine, keys):
    """"param_set" active, wrong levels, out == in of the rotation, out-of-range recorded numbers: -1, nothing reaches the device"""
    api, lib = engine.api, engine.lib
    count = 3
    rng = np.random.default_rng(800)
    c = random_trlwes(rng, count)
    dc = up(engine, c)
    dout = up(engine, np.full(count * 2 * N, FILL, np.uint32))
    d1 = up(engine, np.full(count * (N + 1), FILL, np.uint32))
    d0 = up(engine, np.full(count * (n + 1), FILL, np.uint32))
    dntt = to_ntt(engine, pr.selector(keys, 1))
    e = np.array([1, 2, 3], np.int32)
    j = np.array([1, 2, 3], np.int32)
    trl, trl2, sel, t0, t1 = api.Trlwe(), api.Trlwe(), api.TrgswNtt(), api.Ctxt(0), api.Ctxt(1)
    st = api.Stream()
    st.Create()
    before = api.sched_stats().gates

    def batch_calls():
        return [lib.cufhe_amd_trlwe_rotate_batch(0, None, count, dc.ptr, e.ctypes.data, dout.ptr),
                lib.cufhe_amd_cmux_rotate_batch(0, None, count, dntt.ptr, e.ctypes.data, dc.ptr, dout.ptr),
                lib.cufhe_amd_sample_extract_index_batch(0, None, count, dc.ptr, None, j.ctypes.data, d1.ptr),
                lib.cufhe_amd_sample_extract_index_keyswitch_batch(0, None, count, dc.ptr, None, j.ctypes.data, d0.ptr)]

    def recorded_calls():
        return [lib.cufhe_amd_enqueue_trlwe_op(0, st.st(), api.TL_SEIKS_AT(3), 0, t0._h, trl._h),
                lib.cufhe_amd_enqueue_cmux_rotate(0, st.st(), 0, trl._h, sel._h, trl._h, 5)]

    ps = api.ps_index("default")
    api.ps_initialize(ps, keys.bk, keys.ksk)
    api.set_option("param_set", ps)
    try:
        for rc in batch_calls() + recorded_calls():
            assert rc == -1 and b"param_set" in lib.cufhe_amd_last_error()
    finally:
        api.set_option("param_set", -1)
    # the rotation out of place only
    assert lib.cufhe_amd_trlwe_rotate_batch(0, None, count, dc.ptr, e.ctypes.data, dc.ptr) == -1
    # wrong levels
    assert lib.cufhe_amd_enqueue_trlwe_op(0, st.st(), api.TL_SEIKS_AT(3), 0, t1._h, trl._h) == -1
    assert lib.cufhe_amd_enqueue_trlwe_op(0, st.st(), api.TL_SEIKS_AT(3), 0, t0._h, t0._h) == -1
    assert lib.cufhe_amd_enqueue_cmux_rotate(0, st.st(), 0, trl._h, trl2._h, trl._h, 5) == -1
    assert lib.cufhe_amd_enqueue_cmux_rotate(0, st.st(), 0, t0._h, sel._h, trl._h, 5) == -1
    assert lib.cufhe_amd_enqueue_cmux_rotate(0, st.st(), 0, trl._h, sel._h, sel._h, 5) == -1
    # numbers out of range: nothing recorded
    for bad in (-1, N):
        assert lib.cufhe_amd_enqueue_trlwe_op(0, st.st(), api.TL_SEIKS_AT(bad), 0, t0._h, trl._h) == -1
    for bad in (-1, 2 * N):
        assert lib.cufhe_amd_enqueue_cmux_rotate(0, st.st(), 0, trl._h, sel._h, trl._h, bad) == -1
    assert api.sched_stats().gates == before
    engine.Synchronize()
    assert np.array_equal(dc.download().reshape(count, -1), c)
    for d in (dout, d1, d0):
        assert np.all(d.download() == FILL)
    st.Destroy()


def test_cpp_packed_rom(engine):
    """tests/cpp/test_packed_rom.cpp: the recorded ROM program through include/cufhe_amd.hpp, compared with the oracle it links"""
    exe = pr.build_cpp_program()
    engine.CleanUp()                      # the C++ program owns the device state while it runs
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        k = ol.Keys(ol.load(), seed=1)
        engine.SetGPUNum(1)
        engine.Initialize(k.bk, k.ksk)
