"""GPU tests of circuit bootstrapping (include/cufhe_amd.h: cufhe_amd_cb_*, cufhe_amd_private_keyswitch_batch,
cufhe_amd_circuit_bootstrap_batch, CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP).

Stage words against tests/cb_checker.py (oracle pieces, pinned by tests/test_circuit_bootstrap.py), word for word, no tolerance; the
composition of the stages, TRGSW2NTT and the recorded per-gate API against each other; then a real private key-switching key:
circuit-bootstrapped selectors in CMUXNTT must decrypt correctly, and a 256-entry ROM read recorded as one program returns the
addressed entry.  The measured noise is printed (pytest -s) and asserted against the message margin.
"""
import os
import subprocess

import numpy as np
import pytest

import cb_checker as cb
import oracle_lib as ol

pytestmark = pytest.mark.gpu

N, n = ol.N, ol.n


@pytest.fixture(scope="module")
def keys2(oracle, keys):
    return ol.KeysLvl2(oracle, keys, seed=7)


@pytest.fixture(scope="module")
def engine2(engine, keys2):
    engine.lvl2_initialize(keys2.bk, keys2.ksk)
    return engine


def _upload(eng, arr):
    arr = np.ascontiguousarray(arr)
    if arr.dtype == np.uint64:
        arr = arr.view(np.uint32)
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    return eng.api.DeviceBuffer(arr.size).upload(arr)


# Which private key-switching key the library holds: the word tests use a key of random words, the decryption tests a real one.
# Each test asks for the one it needs (uploaded only on a change), so that any selection or order of the tests works.
_loaded = {"key": None}


def _use(api, name, words):
    if _loaded["key"] != name:
        _loaded["key"] = None
        api.cb_initialize(words)
        _loaded["key"] = name
    return words


def _restore(engine, keys, keys2):
    """the module's device state after a CleanUp: the session keys, the lvl02 key, no private key-switching key"""
    engine.CleanUp()
    _loaded["key"] = None
    engine.SetGPUNum(1)
    engine.Initialize(keys.bk, keys.ksk)
    engine.lvl2_initialize(keys2.bk, keys2.ksk)


@pytest.fixture(scope="module")
def random_words():
    """a private key-switching key of random words: word checks need no encryption"""
    return np.random.default_rng(2024).integers(0, 2**32, size=cb.PKS_KEY_WORDS, dtype=np.uint32)


@pytest.fixture
def random_key(engine2, random_words):
    return _use(engine2.api, "random", random_words)


def test_refusals_without_keys(engine2, keys, keys2, random_words):
    """from a fresh Initialize: without cb_initialize every entry point returns -3 before any device work; with the private key but
    without the lvl02 key the rotations (batch and recorded) return -3 and the stand-alone private key switch runs; a key of the
    wrong size is -1"""
    api = engine2.api
    engine2.CleanUp()
    _loaded["key"] = None
    try:
        engine2.SetGPUNum(1)
        engine2.Initialize(keys.bk, keys.ksk)
        d0 = api.DeviceBuffer(n + 1)
        d2 = api.DeviceBuffer(2 * cb.CB_L * cb.PKS_IN)
        dt = api.DeviceBuffer(cb.TRGSW_WORDS * 2)
        st = api.Stream()
        c0, hold = api.Ctxt(0), api.TrgswNtt()
        for call in (lambda: api.cb_rotate_batch(d0, d2, 1), lambda: api.circuit_bootstrap_batch(d0, 1, trgsw=dt),
                     lambda: api.private_keyswitch_batch(d2, dt, 1), lambda: api.gCircuitBootstrapping(hold, c0, st)):
            with pytest.raises(engine2.CufheAmdError) as e:
                call()
            assert "error -3" in str(e.value) and "cb_initialize" in str(e.value)
        with pytest.raises(engine2.CufheAmdError) as e:
            api.cb_initialize(np.zeros(1000, np.uint32))
        assert "error -1" in str(e.value)
        api.cb_initialize(random_words)
        for call in (lambda: api.cb_rotate_batch(d0, d2, 1), lambda: api.circuit_bootstrap_batch(d0, 1, trgsw=dt),
                     lambda: api.gCircuitBootstrapping(hold, c0, st)):
            with pytest.raises(engine2.CufheAmdError) as e:
                call()
            assert "error -3" in str(e.value) and "lvl2_initialize" in str(e.value)
        d2.upload(np.zeros(d2.words, np.uint32))
        api.private_keyswitch_batch(d2, dt, 1)                 # needs the private key only
        api.Synchronize()
        assert not np.any(dt.download(2 * 2 * N)), "an all-zero input has no nonzero digit"
    finally:
        _restore(engine2, keys, keys2)


@pytest.fixture(params=["quarter_waves", "half_waves"])
def br2_kernel(request, engine2):
    engine2.api.set_option("lvl2_kernel", 1 if request.param == "quarter_waves" else 0)
    yield request.param
    engine2.api.set_option("lvl2_kernel", -1)


@pytest.mark.parametrize("count", [2, 90])
def test_stage1_words(engine2, keys, keys2, random_key, br2_kernel, count):
    """cb_rotate_batch == the checker's rotations at mu_r + mu_r on b, both lvl2 kernels, below and above one rotation per CU
    (90 circuit bootstraps = 270 rotations; a subset of them is checked word for word)"""
    rng = np.random.default_rng(40 + count)
    bits = rng.integers(0, 2, size=count).astype(np.uint8)
    tl = keys.encrypt(bits, 0, seed=400 + count)
    tl[0, n] = 0                                             # bbar = 2N
    d0 = _upload(engine2, tl)
    d2 = engine2.api.DeviceBuffer(count * cb.CB_L * cb.PKS_IN * 2)
    engine2.api.cb_rotate_batch(d0, d2, count)
    got = d2.download().view(np.uint64).reshape(count, cb.CB_L, cb.PKS_IN)
    idx = list(range(count)) if count <= 4 else [0, 1, count // 2, count - 1]
    want = cb.cb_rotate_batch(keys2, tl[idx])
    for k, g in enumerate(idx):
        assert np.array_equal(got[g], want[k]), f"stage 1 of circuit bootstrap {g} differs ({br2_kernel})"


def _stage2_inputs(count, distinct, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 2**64, size=(distinct, cb.PKS_IN), dtype=np.uint64)
    base[0] = 0                                              # every digit zero
    if distinct > 1:
        base[1] = np.uint64(2**64 - 1)                       # every word 0xFFFF...
    if distinct > 2:
        base[2, :] = np.uint64(1 << 33) - np.uint64(1)       # just below the rounding step
    return base, np.arange(count) % distinct


@pytest.mark.parametrize("count, cus", [pytest.param(c, 0, id=str(c)) for c in (1, 3, 24, 257, 3 * 4096)] +
                         [pytest.param(c, cus, id=f"{c}-cus{cus}") for c in (64, 65) for cus in (40, 104)])
def test_stage2_words(engine2, random_key, count, cus):
    """private_keyswitch_batch == the numpy gather-sum mod 2^32.  Large counts repeat a set of distinct inputs (67: not a divisor of
    the tile of 64), so every output is checked at every tile edge and every split-i shape.  The key switch has no slice option:
    one full tile, and one full tile plus a tile of one input, run under "cus_override" 40 and 104, which cut i into 10 / 26 slices
    for one tile and 5 / 13 for two (plan_table_sum with two key functions)"""
    distinct = min(count, 67)
    base, which = _stage2_inputs(count, distinct, seed=count)
    d2 = _upload(engine2, base[which])
    dout = engine2.api.DeviceBuffer(count * 2 * 2 * N)
    engine2.api.set_option("cus_override", cus)
    try:
        engine2.api.private_keyswitch_batch(d2, dout, count)
        got = dout.download().reshape(count, 2, 2, N)
    finally:
        engine2.api.set_option("cus_override", 0)
    want = cb.private_keyswitch_batch(random_key, base)
    assert np.array_equal(got, want[which]), f"private key switch words differ at count {count}, cus_override {cus}"


def test_composition_and_ntt_and_recorded(engine2, keys, random_key):
    """circuit_bootstrap_batch torus words == stage 2 of stage 1; its NTT output == trgsw_to_ntt_batch of the torus words; the
    recorded per-gate op (level-3 holders) == the batch result"""
    api = engine2.api
    count = 5
    rng = np.random.default_rng(77)
    tl = keys.encrypt(rng.integers(0, 2, size=count).astype(np.uint8), 0, seed=770)
    d0 = _upload(engine2, tl)
    d2 = api.DeviceBuffer(count * cb.CB_L * cb.PKS_IN * 2)
    api.cb_rotate_batch(d0, d2, count)
    stage1 = d2.download().view(np.uint64).reshape(count, cb.CB_L, cb.PKS_IN)
    dt = api.DeviceBuffer(count * cb.TRGSW_WORDS)
    dn = api.DeviceBuffer(count * cb.TRGSW_WORDS * 2)
    api.circuit_bootstrap_batch(d0, count, trgsw=dt, trgsw_ntt=dn)
    torus = dt.download().reshape(count, 2 * cb.CB_L, 2, N)
    assert np.array_equal(torus, cb.trgsw_from_stage1(random_key, stage1)), "torus TRGSW != PrivKS of stage 1"
    dn2 = api.DeviceBuffer(count * cb.TRGSW_WORDS * 2)
    api.trgsw_to_ntt_batch(dt, dn2, count)
    ntt = dn.download()
    assert np.array_equal(ntt, dn2.download()), "NTT-domain output != trgsw_to_ntt_batch of the torus output"
    dn3 = api.DeviceBuffer(count * cb.TRGSW_WORDS * 2)
    api.circuit_bootstrap_batch(d0, count, trgsw_ntt=dn3)     # torus words in the library's scratch only
    assert np.array_equal(ntt, dn3.download())
    # recorded: copying form (host words in, NTT words delivered to trgswhost) and device form in one program
    st = api.Stream()
    ins = [api.Ctxt(0) for _ in range(count)]
    outs = [api.TrgswNtt() for _ in range(count)]
    outs_dev = [api.TrgswNtt() for _ in range(count)]
    for g in range(count):
        ins[g].tlwehost[:] = tl[g]
        api.CircuitBootstrapping(outs[g], ins[g], st)
        api.gCircuitBootstrapping(outs_dev[g], ins[g], st)
    api.Synchronize()
    want = ntt.reshape(count, -1)
    for g in range(count):
        assert np.array_equal(outs[g].trgswhost, want[g]), f"recorded circuit bootstrap {g} != batch"
    api.CtxtCopyD2H(outs_dev[0], st)
    api.Synchronize()
    assert np.array_equal(outs_dev[0].trgswhost, want[0])


def test_recorded_refusals(engine2, random_key):
    """wrong holder level, wrong input level, "param_set" active: -1 before anything is recorded"""
    api = engine2.api
    st = api.Stream()
    c0, c1, t = api.Ctxt(0), api.Ctxt(1), api.TrgswNtt()
    tr = api.Trlwe()
    for out, inp in ((tr, c0), (t, c1)):
        with pytest.raises(engine2.CufheAmdError) as e:
            api.gCircuitBootstrapping(out, inp, st)
        assert "error -1" in str(e.value)
    api.set_option("param_set", api.ps_index("k2n512"))
    try:
        with pytest.raises(engine2.CufheAmdError) as e:
            api.gCircuitBootstrapping(t, c0, st)
        assert "error -1" in str(e.value) and "param_set" in str(e.value)
    finally:
        api.set_option("param_set", -1)
    api.Synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# a real private key-switching key
# ---------------------------------------------------------------------------------------------------------------------------------
ALPHA_WORDS = 2.0 ** -25 * 2.0 ** 32          # ORC_ALPHA1 in 32-bit torus words


def _a_times_s(api, s1, a):
    """negacyclic a * s1 mod 2^32 for rows of a ([m][N] uint32) by cufhe_amd_polymul_batch, s1 as int32 0/1"""
    m = a.shape[0]
    chunk = 32768
    out = np.empty_like(a)
    s_rep = np.broadcast_to(s1.astype(np.int32), (chunk, N))
    da = api.DeviceBuffer(chunk * N)
    db = api.DeviceBuffer(chunk * N)
    dr = api.DeviceBuffer(chunk * N)
    da.upload(np.ascontiguousarray(s_rep))
    for o in range(0, m, chunk):
        k = min(chunk, m - o)
        db.upload(a[o:o + k])
        api.polymul_batch(da, db, dr, k)
        out[o:o + k] = dr.download(k * N).reshape(k, N)
    return out


def _negacyclic_schoolbook(a, s):
    res = np.zeros(N, np.int64)
    for j in np.nonzero(s)[0]:
        r = np.roll(a.astype(np.int64), j)
        r[:j] = -r[:j]
        res += r
    return (res & 0xFFFFFFFF).astype(np.uint32)


@pytest.fixture(scope="module")
def real_words(engine2, keys, keys2):
    """K[u][i][j][v-1] = TRLWE_s1(v k2_i 2^(32 - 3 (j + 1)) f_u), f_0 = -s1(X), f_1 = 1, k2_i = s2[i], k2_N2 = -1, alpha = 2^-25"""
    api = engine2.api
    s1 = keys.s1.astype(np.int64)
    rng = np.random.default_rng(99)
    rows = cb.PKS_IN * cb.PKS_T * cb.PKS_NUMBASE
    a = rng.integers(0, 2**32, size=(2 * rows, N), dtype=np.uint32)
    asb = _a_times_s(api, keys.s1, a)
    for r in (0, 12345, 2 * rows - 1):                        # spot checks of the GPU products
        assert np.array_equal(asb[r], _negacyclic_schoolbook(a[r], s1))
    k2 = np.concatenate([keys2.s2.astype(np.int64), [-1]])
    i, j, v = np.meshgrid(np.arange(cb.PKS_IN), np.arange(cb.PKS_T), np.arange(1, cb.PKS_NUMBASE + 1), indexing="ij")
    c = (v * k2[i] * (1 << 32 - 3 * (j + 1))).reshape(-1) & 0xFFFFFFFF                    # [rows]
    e = np.rint(rng.normal(0.0, ALPHA_WORDS, size=(2 * rows, N))).astype(np.int64)
    b = asb.astype(np.int64) + e
    del e, asb
    b = b.reshape(2, rows, N)
    b[1, :, 0] += c                                                                         # f_1 = 1
    b[0] -= (c[:, None] * s1[None, :])                                                      # f_0 = -s1(X)
    key = np.empty((2, rows, 2, N), np.uint32)
    key[:, :, 0, :] = a.reshape(2, rows, N)
    key[:, :, 1, :] = (b & 0xFFFFFFFF).astype(np.uint32)
    del a, b
    return key.reshape(-1)


@pytest.fixture
def real_key(engine2, real_words):
    return _use(engine2.api, "real", real_words)


def _trlwe(api, s1, msgs, seed):
    """TRLWE_s1 encryptions of message polynomials [m][N] (torus words), noise alpha = 2^-25"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2**32, size=msgs.shape, dtype=np.uint32)
    b = _a_times_s(api, s1, a).astype(np.int64) + msgs + np.rint(rng.normal(0.0, ALPHA_WORDS, size=msgs.shape)).astype(np.int64)
    return np.stack([a, (b & 0xFFFFFFFF).astype(np.uint32)], axis=1)


def _phase(api, s1, ct):
    """b - a s1 of TRLWEs [m][2][N], as signed 32-bit words"""
    p = (ct[:, 1].astype(np.int64) - _a_times_s(api, s1, np.ascontiguousarray(ct[:, 0])).astype(np.int64)) & 0xFFFFFFFF
    return np.where(p >= 2**31, p - 2**32, p)


def test_cmux_with_circuit_bootstrapped_selectors(engine2, keys, real_key):
    """1024 random bits -> CB -> CMUX between two known TRLWEs: every coefficient decrypts to the selected message"""
    api = engine2.api
    count = 1024
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, size=count).astype(np.uint8)
    tl = keys.encrypt(bits, 0, seed=505)
    m1 = np.where(rng.integers(0, 2, size=(count, N)) == 1, 1 << 29, -(1 << 29)).astype(np.int64)
    m0 = np.where(rng.integers(0, 2, size=(count, N)) == 1, 1 << 29, -(1 << 29)).astype(np.int64)
    c1 = _trlwe(api, keys.s1, m1, 11)
    c0 = _trlwe(api, keys.s1, m0, 12)
    d0 = _upload(engine2, tl)
    dn = api.DeviceBuffer(count * cb.TRGSW_WORDS * 2)
    api.circuit_bootstrap_batch(d0, count, trgsw_ntt=dn)
    dc1, dc0 = _upload(engine2, c1), _upload(engine2, c0)
    dres = api.DeviceBuffer(count * 2 * N)
    api.cmux_batch(dn, dc1, dc0, dres, count)
    res = dres.download().reshape(count, 2, N)
    ph = _phase(api, keys.s1, res)
    want = np.where(bits[:, None] == 1, m1, m0)
    err = ph - want
    sigma, mx = float(np.std(err)) / 2**32, float(np.max(np.abs(err))) / 2**32
    print(f"\nCB + 1 CMUX: phase error sigma 2^{np.log2(sigma):.2f}, max 2^{np.log2(mx):.2f} (margin 2^-3)")
    assert mx < 2.0 ** -3, "a coefficient decrypts wrongly"
    assert np.array_equal(np.sign(ph), np.sign(want))


def test_rom_read_recorded_program(engine2, keys, real_key):
    """a 256-entry ROM of lvl1 TRLWEs; 8 address bits made by lvl0 gates (XOR of two encrypted bits), circuit-bootstrapped, then a
    255-CMUX tree in 8 levels -- recorded as ONE program through the per-gate API, for 32 random addresses at once"""
    api = engine2.api
    A, R = 32, 256
    rng = np.random.default_rng(17)
    rom_msgs = np.where(rng.integers(0, 2, size=(R, N)) == 1, 1 << 29, -(1 << 29)).astype(np.int64)
    rom_ct = _trlwe(api, keys.s1, rom_msgs, 21)
    addrs = rng.integers(0, R, size=A)
    st = api.Stream()
    rom = []
    for r in range(R):
        t = api.Trlwe()
        t.trlwehost[:] = rom_ct[r].reshape(-1)
        api.CtxtCopyH2D(t, st)
        rom.append(t)
    keep, results = [], []
    for a_i, addr in enumerate(addrs):
        bits = np.array([(addr >> k) & 1 for k in range(8)], np.uint8)
        mask = rng.integers(0, 2, size=8).astype(np.uint8)
        xa = keys.encrypt(bits ^ mask, 0, seed=1000 + a_i)
        xb = keys.encrypt(mask, 0, seed=2000 + a_i)
        sels = []
        for k in range(8):
            ca, cb_, cx = api.Ctxt(0), api.Ctxt(0), api.Ctxt(0)
            ca.tlwehost[:] = xa[k]
            cb_.tlwehost[:] = xb[k]
            api.Xor(cx, ca, cb_, st)
            s = api.TrgswNtt()
            api.gCircuitBootstrapping(s, cx, st)
            sels.append(s)
            keep += [ca, cb_, cx]
        level = rom
        for k in range(8):
            nxt = []
            for j in range(len(level) // 2):
                o = api.Trlwe()
                api.gCMUXNTT(o, sels[k], level[2 * j + 1], level[2 * j], st)
                nxt.append(o)
            keep += level if level is not rom else []
            level = nxt
        api.CtxtCopyD2H(level[0], st)
        results.append(level[0])
        keep += sels
    api.Synchronize()
    got = np.stack([r.trlwehost.reshape(2, N) for r in results])
    ph = _phase(api, keys.s1, got)
    want = rom_msgs[addrs]
    err = ph - want
    sigma, mx = float(np.std(err)) / 2**32, float(np.max(np.abs(err))) / 2**32
    print(f"\nROM read, 8 CMUX levels: phase error sigma 2^{np.log2(sigma):.2f}, max 2^{np.log2(mx):.2f} (margin 2^-3)")
    assert np.array_equal(np.sign(ph), np.sign(want)), "the ROM read returned a wrong entry"
    assert mx < 2.0 ** -3, "a coefficient is outside the message margin"


def _build_cpp_program():
    """tests/cpp/test_circuit_bootstrap.cpp -> tests/cpp/test_circuit_bootstrap, flags as for the other C++ test programs"""
    import cpp_build
    cdefs, libs = cpp_build.hip_flags()
    root = ol.ROOT
    exe = os.path.join(root, "tests", "cpp", "test_circuit_bootstrap")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + cdefs +
                          ["-o", exe, os.path.join(root, "tests", "cpp", "test_circuit_bootstrap.cpp"),
                           "-L" + os.path.join(root, "cufhe_amd"), "-lcufhe_amd", "-Wl,-rpath," + os.path.join(root, "cufhe_amd")] + libs)
    return exe


def test_cpp_rom_read_on_streams(engine2, keys, keys2, real_words, tmp_path):
    """tests/cpp/test_circuit_bootstrap.cpp: a 16-entry ROM read for 8 addresses through include/cufhe_amd.hpp -- CircuitBootstrapping
    into cuFHETRGSWNTTlvl1, CMUXNTT / gCMUXNTT on Streams; the roots decrypt to the addressed entries"""
    api = engine2.api
    bits, A = 4, 8
    R = 1 << bits
    rng = np.random.default_rng(23)
    rom_msgs = np.where(rng.integers(0, 2, size=(R, N)) == 1, 1 << 29, -(1 << 29)).astype(np.int64)
    rom_ct = _trlwe(api, keys.s1, rom_msgs, 31)
    addrs = rng.integers(0, R, size=A)
    addr_bits = np.array([[(a >> k) & 1 for k in range(bits)] for a in addrs], np.uint8)
    addr_ct = keys.encrypt(addr_bits.reshape(-1), 0, seed=33)
    d = tmp_path
    keys.bk.tofile(d / "bk.u32")
    keys.ksk.tofile(d / "ksk.u32")
    keys2.bk.tofile(d / "bk2.u64")
    keys2.ksk.tofile(d / "ksk2.u32")
    real_words.tofile(d / "pksk.u32")
    rom_ct.astype(np.uint32).tofile(d / "rom.u32")
    addr_ct.astype(np.uint32).tofile(d / "addr.u32")
    exe = _build_cpp_program()
    engine2.CleanUp()                      # the C++ program owns the device state while it runs
    _loaded["key"] = None
    try:
        out = subprocess.run([exe, str(d), str(bits), str(A)], capture_output=True, text=True, timeout=600)
        print(out.stdout[-2000:])
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        (d / "pksk.u32").unlink()
        _restore(engine2, keys, keys2)
    got = np.fromfile(d / "out.u32", np.uint32).reshape(A, 2, N)
    ph = _phase(api, keys.s1, got)
    want = rom_msgs[addrs]
    mx = float(np.max(np.abs(ph - want))) / 2**32
    print(f"C++ ROM read, {bits} CMUX levels: max phase error 2^{np.log2(mx):.2f}")
    assert np.array_equal(np.sign(ph), np.sign(want)), "the C++ ROM read returned a wrong entry"
    assert mx < 2.0 ** -3


def test_refusal_with_param_set_and_fail_alloc(engine2, keys, real_key):
    """"param_set" active: -1 before device work; a failed cb_initialize ("test_fail_alloc") leaves the loaded key usable"""
    api = engine2.api
    d0 = _upload(engine2, keys.encrypt(np.array([1], np.uint8), 0, seed=3))
    dn = api.DeviceBuffer(cb.TRGSW_WORDS * 2)
    api.circuit_bootstrap_batch(d0, 1, trgsw_ntt=dn)
    before = dn.download()
    api.set_option("test_fail_alloc", 0)
    with pytest.raises(engine2.CufheAmdError):
        api.cb_initialize(np.zeros(cb.PKS_KEY_WORDS, np.uint32))
    api.set_option("test_fail_alloc", -1)
    dn2 = api.DeviceBuffer(cb.TRGSW_WORDS * 2)
    api.circuit_bootstrap_batch(d0, 1, trgsw_ntt=dn2)
    assert np.array_equal(before, dn2.download())
    idx = api.ps_index("k2n512")
    api.set_option("param_set", idx)
    try:
        with pytest.raises(engine2.CufheAmdError) as e:
            api.circuit_bootstrap_batch(d0, 1, trgsw_ntt=dn2)
        assert "error -1" in str(e.value)
    finally:
        api.set_option("param_set", -1)
