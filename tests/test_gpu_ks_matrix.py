"""GPU tests of the lvl10 key switch as an int8 matrix product (keyswitch_mm_kernel, cufhe_amd/csrc/kernels_ks2.hip.h; arithmetic:
tests/test_ks_matrix.py).  Every case runs with "ks_mm_threshold" 1 (the matrix kernel at any count), is compared word for word with
the CPU oracle, and again with the same call under "ks_mm_threshold" 0 (the kernels the launch rules choose otherwise).

R = kKsMmRows is the rows of one workgroup tile: count 1 is a tile with one live row, R a full tile, R + 1 a second tile with one live
row.  Outputs are packed at 631 words per row, so a store into a pad column (words 631..639 of the last 32-word block) would show
up as a wrong word 0..8 of the next row or in the guard behind the last one (tests/footprint.py: Arena).  The kernel adds nothing
with atomics -- a workgroup owns its words and walks all of K -- so there is no ordering to test."""
import contextlib
import ctypes

import numpy as np
import pytest

import footprint as fp
import oracle_lib as ol
import positions as pos

pytestmark = pytest.mark.gpu

N, n = ol.N, ol.n
W0, W1 = n + 1, N + 1
U32 = np.uint32
R = fp.csrc_constant("kKsMmRows", ("kernels_ks2.hip.h",))
COUNTS = (1, R, R + 1)
NAND, XOR = ol.OPS.index("NAND"), ol.OPS.index("XOR")
# iksoffsetgen + roundoffset of the lvl10 key switch (KsShapeDefault::koff): the digit word of a'_j is (a'_j + KOFF) >> 16
KOFF = (1 << 15) + sum(2 << (32 - 2 * i) for i in range(1, 9))
CARRY_KEYS = (0x80808080, 0x7FFFFFFF, 0xFFFFFFFF)


def rnd(seed, shape):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(U32)


class DeviceBackend:
    def __init__(self, api):
        self.api = api

    def alloc(self, words):
        self.buf = self.api.DeviceBuffer(words)
        return self.buf.ptr

    def upload(self, host):
        self.buf.upload(host)

    def download(self):
        return self.buf.download()


@contextlib.contextmanager
def mm_threshold(api, value):
    try:
        api.set_option("ks_mm_threshold", value)
        yield
    finally:
        api.set_option("ks_mm_threshold", -1)


def a_of_digit_word(dw):
    """a value a'_j whose digit word is dw (low bits in the middle of the rounding interval)"""
    return ((dw << 16) + 0x8000 - KOFF) & 0xFFFFFFFF


def field_inputs():
    """rows of lvl1 ciphertexts: every field 0, every field 1, every field 3; then one row per field value 0..3 of the single
    (j, kappa) = (517, 5) -- an odd j in the upper lane half, a field in the digit word's low byte -- all other fields 2"""
    rows = np.zeros((7, W1), U32)
    for i, f in enumerate((0, 1, 3)):
        rows[i, :N] = a_of_digit_word(0x5555 * f)
    for f in range(4):
        rows[3 + f, :N] = a_of_digit_word(0xAAAA)
        rows[3 + f, 517] = a_of_digit_word((0xAAAA & ~(3 << (14 - 2 * 5))) | (f << (14 - 2 * 5)))
    rows[:, N] = rnd(31, 7)
    return rows


def keyswitch_arena(api, lib, tlwe1, label):
    """one cufhe_amd_keyswitch_batch over an Arena: the output rows, after the footprint check"""
    count = tlwe1.shape[0]
    arena = fp.Arena(label, [fp.Operand("tlwe1", U32, count, W1, "in"), fp.Operand("tlwe0", U32, count, W0, "out")], DeviceBackend(api))
    try:
        arena.set("tlwe1", tlwe1)
        arena.upload()
        rc = lib.cufhe_amd_keyswitch_batch(0, None, count, arena.ptr("tlwe1"), arena.ptr("tlwe0"))
        sync = lib.cufhe_amd_synchronize()
        after = arena.download()
    finally:
        arena.backend.buf.free()
    if rc == -2 or sync != 0:
        pytest.exit(f"{label}: status {rc}, synchronize {sync}: {lib.cufhe_amd_last_error().decode()}", returncode=3)
    assert rc == 0, lib.cufhe_amd_last_error().decode()
    msg = arena.check(after)
    assert msg is None, msg
    return arena.rows(after, "tlwe0")


def both_kernels(api, lib, tlwe1, want, label):
    with mm_threshold(api, 1):
        got = keyswitch_arena(api, lib, tlwe1, label + ", matrix kernel")
    with mm_threshold(api, 0):
        old = keyswitch_arena(api, lib, tlwe1, label + ", existing kernel")
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{label}: rows {bad[:10].tolist()} differ from the oracle; row {bad[0]} words {np.flatnonzero(got[bad[0]] != want[bad[0]])[:10].tolist()}"
    assert np.array_equal(got, old), f"{label}: differs from the existing kernel"


@pytest.fixture(scope="module")
def random_rows(keys):
    """R + 1 distinct random lvl1 ciphertexts (rows 0 and 1: all zero, all ones) and their key switch by the oracle"""
    t1 = rnd(4100, (R + 1, W1))
    t1[0], t1[1] = 0, 0xFFFFFFFF
    return t1, np.stack([keys.keyswitch(r) for r in t1])


@pytest.mark.parametrize("count", COUNTS)
def test_keyswitch_batch(engine, keys, random_rows, count):
    t1, want = random_rows
    # the live row of a tile of one is the LAST distinct row at count R + 1: take the rows from the end so that it is a random one
    both_kernels(engine.api, engine.lib, t1[R + 1 - count:], want[R + 1 - count:], f"keyswitch_batch, count {count}")


@pytest.mark.parametrize("op", [NAND, XOR], ids=["NAND", "XOR"])
def test_gate_level0_output_stride_632(engine, keys, op):
    """the key switch behind a level-0 gate writes through the caller's stride: 632 words, so the row starts drift through all four
    alignments and a pad-column store would land in the pad word or the next row"""
    api, lib = engine.api, engine.lib
    count, stride = R + 1, W0 + 1
    bits = np.random.default_rng(5).integers(0, 2, size=(2, count)).astype(np.uint8)
    ins = [keys.encrypt(bits[i], 0, 50 + i) for i in range(2)]
    want = keys.gate_batch(op, 0, ins[0], ins[1])
    ops = np.array([op], np.int32)
    outs = []
    for thr in (1, 0):
        arena = fp.Arena(f"gate_batch level 0, stride {stride}, ks_mm_threshold {thr}",
                         [fp.Operand("out", U32, count, W0, "out", stride)] + [fp.Operand(k, U32, count, W0, "in", stride) for k in ("in0", "in1")],
                         DeviceBackend(api))
        try:
            arena.set("in0", ins[0])
            arena.set("in1", ins[1])
            arena.upload()
            with mm_threshold(api, thr):
                rc = lib.cufhe_amd_gate_batch(0, None, 0, count, ops.ctypes.data, 0, arena.ptr("out"), arena.ptr("in0"), arena.ptr("in1"), None, stride)
                sync = lib.cufhe_amd_synchronize()
            after = arena.download()
        finally:
            arena.backend.buf.free()
        if rc == -2 or sync != 0:
            pytest.exit(f"{arena.label}: status {rc}, synchronize {sync}: {lib.cufhe_amd_last_error().decode()}", returncode=3)
        assert rc == 0, lib.cufhe_amd_last_error().decode()
        msg = arena.check(after)
        assert msg is None, msg
        outs.append(arena.rows(after, "out"))
    assert np.array_equal(outs[0], want), "matrix kernel: differs from the oracle"
    assert np.array_equal(outs[0], outs[1]), "matrix kernel: differs from the existing kernel"


@pytest.fixture
def carry_engine(engine, keys, oracle):
    """Initialize with a key of one constant word; the session's key is back when the test ends"""
    made = []          # (evaluation key, its key words): the oracle's key points at the array it was made from

    def use(word):
        ksk = np.full(ol.KSK_WORDS, word, U32)
        ek = oracle.orc_evalkey_create(keys.bk, ksk)
        made.append((ek, ksk))
        engine.Initialize(keys.bk, ksk)
        return ek
    yield use
    for ek, _ in made:
        oracle.orc_evalkey_destroy(ek)
    engine.Initialize(keys.bk, keys.ksk)


@pytest.mark.parametrize("word", CARRY_KEYS, ids=[f"{w:#x}" for w in CARRY_KEYS])
def test_carry_keys(engine, oracle, carry_engine, random_rows, word):
    """keys whose every word is all carries (0x80808080: digits -128, -127, -127, -127), the largest positive word and -1, under
    digit words that add every row (all fields 0 or 1: |plane sum| up to 2^20), subtract every row (all fields 3) and touch one row"""
    ek = carry_engine(word)

    def ks(row):
        out = np.zeros(W0, U32)
        oracle.orc_keyswitch(ek, out, np.ascontiguousarray(row, U32))
        return out
    special = field_inputs()
    t1 = np.concatenate([special, random_rows[0][:R + 1 - special.shape[0]]])
    want = np.stack([ks(r) for r in t1])
    # with a constant key the words 0..629 of a row are all equal: the sums are checked, the column routing by the other tests
    for count in COUNTS:
        both_kernels(engine.api, engine.lib, t1[:count], want[:count], f"key {word:#x}, count {count}")
    # the tile of one live row with each of the special rows in turn
    for i in range(1, special.shape[0]):
        both_kernels(engine.api, engine.lib, t1[i:i + 1], want[i:i + 1], f"key {word:#x}, row {i} alone")


@pytest.mark.parametrize("op", [NAND, XOR], ids=["NAND", "XOR"])
def test_gate_level1(engine, keys, op):
    """gate_batch at level 1: the key switch comes first with the gate's linear pre-add (ca, cb, offset) in force"""
    api = engine.api
    count = R + 1
    bits = np.random.default_rng(6).integers(0, 2, size=(2, count)).astype(np.uint8)
    ins = [keys.encrypt(bits[i], 1, 60 + i) for i in range(2)]
    want = keys.gate_batch(op, 1, ins[0], ins[1])
    d_in = [api.DeviceBuffer(count * W1) for _ in range(2)]
    d_out = api.DeviceBuffer(count * W1)
    got = []
    try:
        for i in range(2):
            d_in[i].upload(ins[i])
        for thr in (1, 0):
            d_out.upload(pos.poison(count * W1))
            with mm_threshold(api, thr):
                api.gate_batch(op, 1, d_out, d_in[0], d_in[1], count=count)
                engine.Synchronize()
            got.append(d_out.download().reshape(count, W1))
    finally:
        for d in d_in + [d_out]:
            d.free()
    assert np.array_equal(got[0], want), "matrix kernel: differs from the oracle"
    assert np.array_equal(got[0], got[1]), "matrix kernel: differs from the existing kernel"


def test_full_batch_default_rule(engine, keys):
    """4096 key switches through the default rule (no option set): 32 sampled rows against the oracle, all rows against the existing kernel"""
    api = engine.api
    count = 4096
    t1 = rnd(77, (count, W1))
    d_in, d_out = api.DeviceBuffer(count * W1), api.DeviceBuffer(count * W0)
    try:
        d_in.upload(t1)
        d_out.upload(pos.poison(count * W0))
        api.keyswitch_batch(d_in, d_out, count)
        engine.Synchronize()
        got = d_out.download().reshape(count, W0)
        d_out.upload(pos.poison(count * W0))
        with mm_threshold(api, 0):
            api.keyswitch_batch(d_in, d_out, count)
            engine.Synchronize()
        old = d_out.download().reshape(count, W0)
    finally:
        d_in.free()
        d_out.free()
    fixed = [0, R - 1, R, count - 1]
    rows = fixed + [g for g in np.random.default_rng(8).permutation(count).tolist() if g not in fixed][:32 - len(fixed)]
    for g in rows:
        assert np.array_equal(got[g], keys.keyswitch(t1[g])), f"row {g} differs from the oracle"
    assert np.array_equal(got, old), "differs from the existing kernel"
