"""GPU tests of TLWE packing.  Word parity is equality of every word of every output with
tests/pack_checker.py under a key of random words (parity needs no valid key), at every launch shape plan::plan_pack can return;
one end-to-end case under a genuine key is the RAM-write path: gate results packed on the device, CMUXed against a host-encrypted
word, extracted and decrypted.  The C++ mirror tests/cpp/test_pack.cpp runs last."""
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import pack_checker as pk
import packed_rom_checker as pr

pytestmark = pytest.mark.gpu

N, n = ol.N, ol.n
FILL = 0xA5A5A5A5
COUNTS = [1, 3, 64, 65, 130]           # a single input, a partial tile, a full tile, a one-over tail, two tiles and a partial one
POSITIONS = (0, 1, 511, 1023)
MAX_SLICES = (n + 15) // 16
TRGSW_WORDS = 12 * N
_loaded = [None]


def up(eng, arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    return eng.api.DeviceBuffer(arr.size).upload(arr)


def load_key(eng, name, key):
    if _loaded[0] != name:
        eng.api.pack_initialize(key)
        _loaded[0] = name


@pytest.fixture(scope="module")
def random_key_words(engine):
    """before the first cufhe_amd_pack_initialize of the session: well-formed arguments are refused with -3 and nothing is written"""
    api, lib = engine.api, engine.lib
    zero = np.zeros(2, np.int32)
    if _loaded[0] is None:
        din, dout = up(engine, np.zeros(2 * (n + 1), np.uint32)), up(engine, np.full(2 * N, FILL, np.uint32))
        assert lib.cufhe_amd_pack_batch(0, None, 2, din.ptr, zero.ctypes.data, zero.ctypes.data, 1, dout.ptr) == -3
        assert b"cufhe_amd_pack_initialize" in lib.cufhe_amd_last_error()
        engine.Synchronize()
        assert np.all(dout.download() == FILL)
    return np.random.default_rng(900).integers(0, 1 << 32, size=pk.KEY_WORDS, dtype=np.uint64).astype(np.uint32)


@pytest.fixture
def random_key(engine, random_key_words):
    load_key(engine, "random", random_key_words)
    return random_key_words


@pytest.fixture(scope="module")
def genuine_key_words(keys):
    return pk.genuine_key(keys, seed=901)


@pytest.fixture
def genuine_key(engine, genuine_key_words):
    load_key(engine, "genuine", genuine_key_words)
    return genuine_key_words


def targets(rng, count, count_out):
    """dst / pos of `count` inputs.  count_out = 5: output 3 stays unnamed, output 1 is named by every second input, the others share
    0, 2 and 4; the positions cycle through POSITIONS with a random one every fifth input; the last input repeats the (dst, pos) of
    the first (count >= 2)."""
    dst = np.zeros(count, np.int32)
    if count_out > 1:
        others = [o for o in range(count_out) if o not in (1, 3)]
        dst[:] = [1 if m % 2 else others[(m // 2) % len(others)] for m in range(count)]
    pos = np.array([POSITIONS[m % len(POSITIONS)] for m in range(count)], np.int32)
    pos[4::5] = rng.integers(0, N, size=len(pos[4::5]))
    if count >= 2:
        dst[-1], pos[-1] = dst[0], pos[0]
    return dst, pos


_rows = {}


def inputs_and_rows(key, count):
    """the inputs of a case and the checker's PackKS of each, computed once per count and shared by its cases"""
    if count not in _rows:
        x = pk.edge_inputs(np.random.default_rng(1000 + count), count)
        _rows[count] = (x, [pk.pack_ks(key, x[m]) for m in range(count)])
    return _rows[count]


@pytest.mark.parametrize("count_out", [1, 5])
@pytest.mark.parametrize("count", COUNTS)
def test_every_word_at_every_shape(engine, random_key, count, count_out):
    """slices = 1 .. 40 forced by "pack_slices" (every shape of plan_pack: the tiles follow from the count), the automatic rule at the
    device's CU count and at 40 and 104 CUs: all give the checker's words, so the words are identical across shapes"""
    api = engine.api
    x, rows = inputs_and_rows(random_key, count)
    dst, pos = targets(np.random.default_rng(1000 + 10 * count + count_out), count, count_out)
    if count_out == 5:
        assert 3 not in dst and (count < 3 or np.count_nonzero(dst == 1) >= count // 3)      # one unnamed, one named by many
    want = np.zeros((count_out, 2 * N), np.uint32)
    for m in range(count):
        want[dst[m]] += pk.rotate(rows[m], int(pos[m]))
    if count_out == 5:
        assert not want[3].any()
    din = up(engine, x)
    dout = up(engine, np.full(count_out * 2 * N, FILL, np.uint32))
    shapes = [("pack_slices", s) for s in range(1, MAX_SLICES + 1)] + [("pack_slices", -1), ("cus_override", 40), ("cus_override", 104)]
    try:
        for key, value in shapes:
            api.set_option(key, value)
            dout.upload(np.full(count_out * 2 * N, FILL, np.uint32))
            api.pack_batch(din, dst, pos, dout, count, count_out)
            engine.Synchronize()
            got = dout.download().reshape(count_out, 2 * N)
            bad = np.argwhere(got != want)
            assert bad.size == 0, f"{key} = {value}: {len(bad)} words differ, first at (output, word) {tuple(bad[0])}"
            api.set_option(key, -1 if key == "pack_slices" else 0)
    finally:
        api.set_option("pack_slices", -1)
        api.set_option("cus_override", 0)
    assert np.array_equal(din.download().reshape(count, -1), x)


def test_no_inputs_zeroes_the_outputs(engine, random_key):
    dout = up(engine, np.full(3 * 2 * N, FILL, np.uint32))
    din = up(engine, np.zeros(n + 1, np.uint32))
    e = np.zeros(1, np.int32)
    engine.check(engine.lib.cufhe_amd_pack_batch(0, None, 0, din.ptr, e.ctypes.data, e.ctypes.data, 3, dout.ptr))
    engine.Synchronize()
    assert not dout.download().any()


def test_refusals_leave_the_outputs_untouched(engine, keys, random_key):
    api, lib = engine.api, engine.lib
    count = 3
    x = pk.edge_inputs(np.random.default_rng(1100), count)
    din, dout = up(engine, x), up(engine, np.full(2 * 2 * N, FILL, np.uint32))
    ok = np.zeros(count, np.int32)
    for which, bad in (("dst", -1), ("dst", 2), ("pos", -1), ("pos", N)):
        d, p = ok.copy(), ok.copy()
        (d if which == "dst" else p)[1] = bad
        assert lib.cufhe_amd_pack_batch(0, None, count, din.ptr, d.ctypes.data, p.ctypes.data, 2, dout.ptr) == -1
        assert which.encode() in lib.cufhe_amd_last_error()
    ps = api.ps_index("default")
    api.ps_initialize(ps, keys.bk, keys.ksk)
    api.set_option("param_set", ps)
    try:
        assert lib.cufhe_amd_pack_batch(0, None, count, din.ptr, ok.ctypes.data, ok.ctypes.data, 2, dout.ptr) == -1
        assert b"param_set" in lib.cufhe_amd_last_error() and b"default path only" in lib.cufhe_amd_last_error()
        assert lib.cufhe_amd_pack_initialize(random_key.ctypes.data, random_key.size) == -1
        assert b"param_set" in lib.cufhe_amd_last_error()
    finally:
        api.set_option("param_set", -1)
    engine.Synchronize()
    assert np.all(dout.download() == FILL)
    # the key that was loaded is still in use
    api.pack_batch(din, ok, ok, dout, count, 2)
    engine.Synchronize()
    assert np.array_equal(dout.download().reshape(2, -1), pk.pack_batch(random_key, x, ok, ok, 2))


def to_ntt(eng, trgsw):
    d = up(eng, np.ascontiguousarray(trgsw, np.uint32).ravel())
    dntt = eng.api.DeviceBuffer(TRGSW_WORDS * 2)
    eng.api.trgsw_to_ntt_batch(d, dntt, 1)
    return dntt


def word_trlwe(keys, word, seed):
    """a host-encrypted TRLWE with bit b of `word` at coefficient b, messages +-mu"""
    msgs = np.zeros(N, np.uint32)
    for b in range(8):
        msgs[b] = ol.MU if (word >> b) & 1 else (1 << 32) - ol.MU
    return pr.encrypt_trlwe(keys, msgs, 64.0, seed)


def test_ram_write_end_to_end(engine, keys, genuine_key):
    """eight Xor gates on encrypted bits -> pack_batch of the results at positions 0 .. 7 of one TRLWE -> CMUX against a host-encrypted
    TRLWE under a host-encrypted selector -> indexed extraction with key switch at 0 .. 7 -> the selected word, for both selectors"""
    api = engine.api
    rng = np.random.default_rng(1200)
    a, b = rng.integers(0, 2, size=(2, 8)).astype(np.uint8)
    other = int(rng.integers(0, 256))
    da, db = up(engine, keys.encrypt(a, 0, seed=1201)), up(engine, keys.encrypt(b, 0, seed=1202))
    dx = api.DeviceBuffer(8 * (n + 1))
    api.gate_batch(api.XOR, 0, dx, da, db, count=8)
    dpacked = up(engine, np.full(2 * N, FILL, np.uint32))
    idx = np.arange(8, dtype=np.int32)
    api.pack_batch(dx, np.zeros(8, np.int32), idx, dpacked, 8, 1)
    engine.Synchronize()
    gates = dx.download().reshape(8, -1)
    assert list(keys.decrypt(gates, 0)) == list(a ^ b)
    packed = dpacked.download()
    assert np.array_equal(packed, pk.pack_batch(genuine_key, gates, np.zeros(8, np.int32), idx, 1)[0])
    dother = up(engine, word_trlwe(keys, other, seed=1203))
    for bit in (1, 0):
        dsel = to_ntt(engine, pr.selector(keys, bit))
        dres, dout = api.DeviceBuffer(2 * N), api.DeviceBuffer(8 * (n + 1))
        api.cmux_batch(dsel, dpacked, dother, dres, 1)
        api.sample_extract_index_keyswitch_batch(dres, idx, dout, 8, src=np.zeros(8, np.int32))
        engine.Synchronize()
        got = keys.decrypt(dout.download().reshape(8, -1), 0)
        want = (a ^ b) if bit else np.array([(other >> k) & 1 for k in range(8)], np.uint8)
        assert list(got) == list(want), f"selector of bit {bit}"


def test_object_form_runs_behind_recorded_gates(engine, keys, genuine_key):
    """gPackTLWEs on ciphertext objects: the Xor gates are recorded on the stream and not yet launched when it is called; the packed
    TRLWE is then the operand of recorded operations (indexed extraction) on the same stream"""
    api = engine.api
    rng = np.random.default_rng(1300)
    a, b = rng.integers(0, 2, size=(2, 8)).astype(np.uint8)
    ea, eb = keys.encrypt(a, 0, seed=1301), keys.encrypt(b, 0, seed=1302)
    st = api.Stream()
    st.Create()
    ins = [(api.Ctxt(0), api.Ctxt(0)) for _ in range(8)]
    xs = [api.Ctxt(0) for _ in range(8)]
    for k in range(8):
        ins[k][0].tlwehost[:] = ea[k]
        ins[k][1].tlwehost[:] = eb[k]
        api.Xor(xs[k], ins[k][0], ins[k][1], st)
    packed = api.Trlwe()
    positions = [3 * k + 1 for k in range(8)]
    api.gPackTLWEs(packed, xs, positions, st)
    outs = [api.Ctxt(0) for _ in range(8)]
    for k in range(8):
        api.gSampleExtractAndKeySwitch(outs[k], packed, st, index=positions[k])
        api.CtxtCopyD2H(outs[k], st)
    api.CtxtCopyD2H(packed, st)
    api.Synchronize()
    gates = np.stack([x.tlwehost for x in xs])
    assert list(keys.decrypt(gates, 0)) == list(a ^ b)
    assert np.array_equal(packed.trlwehost, pk.pack_batch(genuine_key, gates, np.zeros(8, np.int32), positions, 1)[0])
    assert list(keys.decrypt(np.stack([o.tlwehost for o in outs]), 0)) == list(a ^ b)
    st.Destroy()


def test_cpp_pack(engine):
    """tests/cpp/test_pack.cpp: the RAM-write path through include/cufhe_amd.hpp"""
    exe = pk.build_cpp_program()
    engine.CleanUp()                      # the C++ program owns the device state while it runs
    _loaded[0] = None
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        k = ol.Keys(ol.load(), seed=1)
        engine.SetGPUNum(1)
        engine.Initialize(k.bk, k.ksk)
