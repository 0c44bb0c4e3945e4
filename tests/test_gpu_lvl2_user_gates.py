"""GPU tests of the user gates of the N = 2048 ring (cufhe_amd_lvl2_define_gate): every comparison is equality with
tests/lvl2_user_gate_checker.py (itself tied to the oracle by tests/test_lvl2_user_gates.py), on both rotation kernels of the ring.
The checker's rotations cost a second or two of CPU each, so every reference is computed once per module and shared by the two
kernels and by the three ways a gate is called."""
import ctypes

import numpy as np
import pytest

import lvl2_user_gate_checker as lc
import oracle_lib as ol

pytestmark = pytest.mark.gpu

n, N2 = ol.n, ol.N2
W0, W2 = n + 1, N2 + 1
FILL = 0xDEADBEEF
NAND, MUX = ol.OPS.index("NAND"), ol.OPS.index("MUX")
P = 8


@pytest.fixture(scope="module")
def keys2(oracle, keys):
    return ol.KeysLvl2(oracle, keys, seed=7)


@pytest.fixture(scope="module")
def engine2(engine, keys2):
    engine.lvl2_initialize(keys2.bk, keys2.ksk)
    return engine


@pytest.fixture(params=["quarter_waves", "half_waves"])
def br2_kernel(request, engine2):
    """both blind-rotate kernels of the ring: four quarter waves per rotation (kernels_lvl2q.hip.h) and eight half waves
    (kernels_lvl2.hip.h); identical words"""
    engine2.api.set_option("lvl2_kernel", 1 if request.param == "quarter_waves" else 0)
    yield request.param
    engine2.api.set_option("lvl2_kernel", -1)


def _tv(seed):
    """a distinct random 64-bit word in every coefficient, with 0, 2^63 and 2^64 - 1 sown in"""
    tv = np.random.default_rng(seed).integers(0, 2**64, N2, dtype=np.uint64)
    tv[[0, 5, N2 - 1]] = [0, 1 << 63, 2**64 - 1]
    tv[[1000, 1024, 2047 - 64]] = [2**64 - 1, 0, 1 << 63]
    assert np.unique(tv[6:1000]).size == 994
    return tv


F_TABLE = np.random.default_rng(77).permutation(P)


class Defs:
    """the module's definitions: every row of the table is taken, rows 0 and 63 carry test vectors"""

    def __init__(self, eng):
        self.tv0, self.tv2, self.tv63 = _tv(1), _tv(2), _tv(63)
        self.values = (F_TABLE.astype(np.uint64) << np.uint64(60)) + np.uint64(12345)
        # (coeffs, offset, tv) by name
        self.spec = {
            "one": ((1, 0, 0), 0, self.tv0),                          # row 0: arity 1 with TV
            "two": ((3, -2, 0), 0x12345678, None),                    # row 1: arity 2, negative c1, an offset, TV NULL
            "three": ((1, -1, 2), 0xF0000001, self.tv2),              # row 2: arity 3 with TV
            "table": ((1, 0, 0), 0, lc.test_vector(self.values)),     # row 3: the p = 8 table of the worked example
            "last": ((-1, 0, 0), 1 << 20, self.tv63),                 # row 63
        }
        self.op = {}
        for name in ("one", "two", "three", "table"):
            c, off, tv = self.spec[name]
            self.op[name] = eng.lvl2_define_gate(c, off, tv)
        for k in range(4, 63):
            assert eng.lvl2_define_gate((1, 1, 0), k) == eng.LVL2_USER_OP_BASE + k
        c, off, tv = self.spec["last"]
        self.op["last"] = eng.lvl2_define_gate(c, off, tv)
        assert [self.op[k] for k in ("one", "two", "three", "table", "last")] == [eng.LVL2_USER_OP_BASE + k for k in (0, 1, 2, 3, 63)]
        self.name_of = {v: k for k, v in self.op.items()}


@pytest.fixture(scope="module")
def defs(engine2):
    return Defs(engine2)


def _upload(eng, arr):
    arr = np.ascontiguousarray(arr)
    if arr.dtype == np.uint64:
        arr = arr.view(np.uint32)
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    return eng.api.DeviceBuffer(arr.size).upload(arr)


def _rotate_inputs(count, seed):
    tl = np.random.default_rng(seed).integers(0, 2**32, size=(8, W0), dtype=np.uint64).astype(np.uint32)
    tl[0, n] = 0                       # bbar = 2 N2: the identity
    tl[1, n] = 0xFFFFFFFF              # bbar = 1
    tl[1, :4] = 0                      # ... and a words 0
    tl[2, n] = 0x80000000              # bbar = N2: every word negated
    tl[2, :8] = 0x7FFFFFFF
    tl[3, n] = 2047 << 20              # bbar = N2 + 1
    tl[4, n] = 1 << 20                 # bbar = 2 N2 - 1
    tl[5, :8] = 0
    tl[6, :8] = 0x7FFFFFFF
    return tl[:count]


_rot_ref = {}


def _rotate_reference(keys2, defs, steps):
    if steps not in _rot_ref:
        count = 4 if steps == 630 else 8
        tl = _rotate_inputs(count, 500 + steps)
        c, off, tv = defs.spec["one"]
        _rot_ref[steps] = (tl, lc.on_threads(lambda g: lc.user_rotate_one(keys2, c, off, tv, [tl[g]], steps), count))
    return _rot_ref[steps]


@pytest.mark.parametrize("steps", [0, 1, 2, 3, 33, 630])
def test_user_rotate_accumulator_words(engine2, keys2, defs, steps, br2_kernel):
    """the accumulator after `steps` steps, started from (0, X^bbar TV); steps 0 is the gather alone, on all 8 inputs"""
    tl, want = _rotate_reference(keys2, defs, steps)
    count = tl.shape[0]
    dacc = engine2.api.DeviceBuffer(count * 2 * N2 * 2)
    engine2.lvl2_user_rotate_batch(defs.op["one"], _upload(engine2, tl), dacc, count, steps=steps)
    got = dacc.download().view(np.uint64).reshape(count, 2 * N2)
    for g in range(count):
        bad = np.flatnonzero(got[g] != want[g])
        assert bad.size == 0, f"rotation {g}: {bad.size} words differ after {steps} steps, first at {bad[:4]}"


def test_user_rotate_of_row_63_and_three_operands(engine2, keys2, defs, br2_kernel):
    """steps 0 and 2 through the last row of the table (negative c0, an offset) and through the pre-added three-operand form"""
    rng = np.random.default_rng(520)
    ins = [rng.integers(0, 2**32, size=(3, W0), dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    d = [_upload(engine2, a) for a in ins]
    for name, steps in (("last", 0), ("last", 2), ("three", 0), ("three", 2)):
        c, off, tv = defs.spec[name]
        dacc = engine2.api.DeviceBuffer(3 * 2 * N2 * 2)
        engine2.lvl2_user_rotate_batch(defs.op[name], d[0], dacc, 3, in1=d[1] if name == "three" else None,
                                       in2=d[2] if name == "three" else None, steps=steps)
        got = dacc.download().view(np.uint64).reshape(3, 2 * N2)
        for g in range(3):
            want = lc.user_rotate_one(keys2, c, off, tv, [a[g] for a in ins], steps)
            assert np.array_equal(got[g], want), (name, steps, g)


# one batch of 16 mixing NAND, MUX and the definitions of arity 1, 2, 3 and of rows 0 and 63
MIX = ["NAND", "MUX", "one", "two", "three", "last", "one", "two", "three", "last", "NAND", "one", "three", "last", "MUX", "two"]
_mix_ref = {}


def _mix(keys2, defs):
    if not _mix_ref:
        rng = np.random.default_rng(540)
        ins = [rng.integers(0, 2**32, size=(len(MIX), W0), dtype=np.uint64).astype(np.uint32) for _ in range(3)]
        ops = np.array([NAND if m == "NAND" else MUX if m == "MUX" else defs.op[m] for m in MIX], np.int32)
        builtin = [g for g, m in enumerate(MIX) if m in ("NAND", "MUX")]
        want = np.zeros((len(MIX), W0), np.uint32)
        want[builtin] = keys2.gate_batch(ops[builtin], ins[0][builtin], ins[1][builtin], ins[2][builtin])
        user = [g for g, m in enumerate(MIX) if m not in ("NAND", "MUX")]
        t2 = lc.on_threads(lambda i: lc.user_extract_one(keys2, *defs.spec[MIX[user[i]]], [a[user[i]] for a in ins]), len(user))
        pre = {}
        for i, g in enumerate(user):
            pre[g] = t2[i]
            want[g] = keys2.keyswitch(t2[i])
        _mix_ref.update(ins=ins, ops=ops, want=want, pre=pre)
    return _mix_ref


def test_gate_words_through_lvl2_gate_batch(engine2, keys2, defs, br2_kernel):
    ref = _mix(keys2, defs)
    d = [_upload(engine2, a) for a in ref["ins"]]
    dout = engine2.api.DeviceBuffer(len(MIX) * W0)
    engine2.lvl2_gate_batch(ref["ops"], dout, d[0], d[1], d[2])
    got = dout.download().reshape(len(MIX), W0)
    for g, m in enumerate(MIX):
        assert np.array_equal(got[g], ref["want"][g]), f"gate {g} ({m}) differs from the checker"


def test_gate_words_at_level_0_with_the_ring_selected(engine2, keys2, defs, br2_kernel):
    """the same ops through cufhe_amd_gate_batch at level 0 and through cufhe_amd_enqueue_gate with "lvl0_ring" 2048"""
    eng, api = engine2, engine2.api
    ref = _mix(keys2, defs)
    api.set_option("lvl0_ring", 2048)
    try:
        d = [_upload(eng, a) for a in ref["ins"]]
        dout = api.DeviceBuffer(len(MIX) * W0)
        eng.gate_batch(ref["ops"], 0, dout, d[0], d[1], d[2], count=len(MIX))
        got = dout.download().reshape(len(MIX), W0)
        for g, m in enumerate(MIX):
            assert np.array_equal(got[g], ref["want"][g]), f"gate_batch: gate {g} ({m}) differs from the checker"
        st = api.Stream()
        st.Create()
        cts = [[api.Ctxt(0) for _ in MIX] for _ in range(4)]
        for g, m in enumerate(MIX):
            for k in range(3):
                cts[k][g].tlwehost[:] = ref["ins"][k][g]
            ar = 2 if m == "NAND" else 3 if m == "MUX" else lc.arity(defs.spec[m][0])
            api.Apply(int(ref["ops"][g]), cts[3][g], *[cts[k][g] for k in range(ar)], st)
        api.Synchronize()
        for g, m in enumerate(MIX):
            assert np.array_equal(cts[3][g].tlwehost, ref["want"][g]), f"enqueue_gate: gate {g} ({m}) differs from the checker"
        st.Destroy()
    finally:
        api.set_option("lvl0_ring", 1024)


@pytest.mark.parametrize("name", ["one", "two", "three", "last"])
def test_extract_words_are_the_gate_before_its_key_switch(engine2, keys2, defs, name, br2_kernel):
    ref = _mix(keys2, defs)
    rows = [g for g, m in enumerate(MIX) if m == name]
    ar = lc.arity(defs.spec[name][0])
    d = [_upload(engine2, ref["ins"][k][rows]) if k < ar else None for k in range(3)]
    dt2 = engine2.api.DeviceBuffer(len(rows) * W2 * 2)
    engine2.lvl2_user_extract_batch(defs.op[name], d[0], dt2, len(rows), in1=d[1], in2=d[2])
    got = dt2.download().view(np.uint64).reshape(len(rows), W2)
    for i, g in enumerate(rows):
        assert np.array_equal(got[i], ref["pre"][g]), f"lvl2 TLWE of gate {g} ({name}) differs from the checker"
    # ... and it is the input form of the ring's key switch
    d0 = engine2.api.DeviceBuffer(len(rows) * W0)
    engine2.lvl2_keyswitch_batch(dt2, d0, len(rows))
    assert np.array_equal(d0.download().reshape(len(rows), W0), ref["want"][rows])


def test_a_batch_without_user_ops_is_the_oracle(engine2, keys, keys2, defs, br2_kernel):
    """with definitions (and their table) present, a batch of built-in gates runs the kernels as they were: orc2_gate_batch's words"""
    ops = np.array([NAND, MUX, ol.OPS.index("XOR"), ol.OPS.index("ORYN"), ol.OPS.index("NMUX"), NAND], np.int32)
    rng = np.random.default_rng(560)
    bits = rng.integers(0, 2, (3, ops.size)).astype(np.uint8)
    cts = [keys.encrypt(bits[i], 0, seed=561 + i) for i in range(3)]
    d = [_upload(engine2, c) for c in cts]
    dout = engine2.api.DeviceBuffer(ops.size * W0)
    engine2.lvl2_gate_batch(ops, dout, d[0], d[1], d[2])
    assert np.array_equal(dout.download().reshape(ops.size, W0), keys2.gate_batch(ops, cts[0], cts[1], cts[2]))


def test_table_gate_decrypts_to_f(engine2, keys, keys2, defs):
    """64 gates of the p = 8 table over all messages: the lvl0 output decrypts to f(m); the lvl2 output's phase is f(m)'s 64-bit word
    within the six-sigma bound of INTEGRATION.md section 5.1"""
    import user_gate_checker as uc
    step = (1 << 32) // (2 * P)
    msgs = np.arange(64) % P
    ins = uc.encrypt_torus(keys, 0, msgs.astype(np.uint64) * np.uint64(step), 2.0 ** -15 * 2.0 ** 32, seed=570)
    din = _upload(engine2, ins)
    dout = engine2.api.DeviceBuffer(64 * W0)
    engine2.lvl2_gate_batch(defs.op["table"], dout, din, count=64)
    ph = uc.phase(keys, 0, dout.download().reshape(64, W0)).astype(np.int64)
    assert np.array_equal(np.rint(ph / float(step)).astype(np.int64) % (2 * P), F_TABLE[msgs])
    dt2 = engine2.api.DeviceBuffer(64 * W2 * 2)
    engine2.lvl2_user_extract_batch(defs.op["table"], din, dt2, 64)
    t2 = dt2.download().view(np.uint64).reshape(64, W2)
    err = np.array([lc.signed64(np.uint64((int(keys2.phase2(t2[g])) - int(defs.values[msgs[g]])) % 2**64)) for g in range(64)])
    s2 = lc.noise_sigmas()[0]
    print(f"lvl2 output over 64 gates: sampled std {err.std():.3e}, max |err| {np.abs(err).max():.3e}, derived sigma {s2:.3e}")
    assert np.abs(err).max() < 6 * s2


def _refused(lib, rc, status, *words):
    msg = lib.cufhe_amd_last_error()
    assert rc == status and msg and all(w in msg for w in words), (rc, msg)


def test_refusals_leave_the_output_untouched(engine2, keys, defs):
    """every refusal returns its status and a message before any device work: the output buffer keeps its fill value"""
    eng, api, lib = engine2, engine2.api, engine2.lib
    count = 3
    a = _upload(eng, np.zeros(count * (ol.N + 1), np.uint32))
    out = api.DeviceBuffer(count * (ol.N + 1)).upload(np.full(count * (ol.N + 1), FILL, np.uint32))
    ops = np.array([NAND, defs.op["two"], NAND], np.int32)
    p = ops.ctypes.data
    # the default ring, level 0 and level 1
    _refused(lib, lib.cufhe_amd_gate_batch(0, None, 0, count, p, 1, out.ptr, a.ptr, a.ptr, a.ptr, W0), -1, b"lvl2 user gates", b"2048")
    _refused(lib, lib.cufhe_amd_gate_batch(0, None, 1, count, p, 1, out.ptr, a.ptr, a.ptr, a.ptr, ol.N + 1), -1, b"lvl2 user gates")
    _refused(lib, lib.cufhe_amd_gate(0, None, defs.op["one"], 0, out.ptr, a.ptr, None, None), -1, b"lvl2 user gates")
    c = [api.Ctxt(0) for _ in range(4)]
    _refused(lib, lib.cufhe_amd_enqueue_gate(0, None, defs.op["two"], 0, c[0]._h, c[1]._h, c[2]._h, None), -1, b"lvl2 user gates")
    arr = (ctypes.c_void_p * 2)(c[0]._h, c[1]._h)
    api.set_option("lvl0_ring", 2048)
    try:
        # level 1 with the ring selected; the multi-output form; a level-1 handle
        _refused(lib, lib.cufhe_amd_gate_batch(0, None, 1, count, p, 1, out.ptr, a.ptr, a.ptr, a.ptr, ol.N + 1), -1, b"lvl2 user gates")
        _refused(lib, lib.cufhe_amd_enqueue_gate_multi(0, None, defs.op["one"], 0, 2, arr, c[2]._h, None, None), -1, b"one output")
        c1 = [api.Ctxt(1) for _ in range(2)]
        _refused(lib, lib.cufhe_amd_enqueue_gate(0, None, defs.op["one"], 0, c1[0]._h, c1[1]._h, None, None), -1, b"lvl2 user gates")
        # missing operands
        _refused(lib, lib.cufhe_amd_gate_batch(0, None, 0, count, p, 1, out.ptr, a.ptr, None, None, W0), -1, b"second operand")
        three = np.array([defs.op["three"]], np.int32)
        _refused(lib, lib.cufhe_amd_lvl2_gate_batch(0, None, count, three.ctypes.data, 0, out.ptr, a.ptr, a.ptr, None, W0), -1, b"third operand")
    finally:
        api.set_option("lvl0_ring", 1024)
    # the hooks: an op outside the range, missing operands, null outputs
    _refused(lib, lib.cufhe_amd_lvl2_user_rotate_batch(0, None, count, NAND, a.ptr, None, None, 0, out.ptr), -1, b"range")
    _refused(lib, lib.cufhe_amd_lvl2_user_rotate_batch(0, None, count, defs.op["two"], a.ptr, None, None, 0, out.ptr), -1, b"second operand")
    _refused(lib, lib.cufhe_amd_lvl2_user_extract_batch(0, None, count, defs.op["three"], a.ptr, a.ptr, None, out.ptr), -1, b"third operand")
    _refused(lib, lib.cufhe_amd_lvl2_user_extract_batch(0, None, count, defs.op["one"], a.ptr, None, None, None), -1, b"null")
    # the 65th definition, c0 = 0, a null op
    coeffs, got = (ctypes.c_int32 * 3)(1, 1, 0), ctypes.c_int(-7)
    _refused(lib, lib.cufhe_amd_lvl2_define_gate(coeffs, 0, None, ctypes.byref(got)), -1, b"full")
    _refused(lib, lib.cufhe_amd_lvl2_define_gate((ctypes.c_int32 * 3)(0, 1, 0), 0, None, ctypes.byref(got)), -1, b"c0")
    _refused(lib, lib.cufhe_amd_lvl2_define_gate(coeffs, 0, None, None), -1, b"null")
    assert got.value == -7
    # "param_set" active: the ops and a definition
    ps = api.ps_index("default")
    api.ps_initialize(ps, keys.bk, keys.ksk)
    api.set_option("param_set", ps)
    try:
        _refused(lib, lib.cufhe_amd_gate_batch(0, None, 0, count, p, 1, out.ptr, a.ptr, a.ptr, a.ptr, W0), -1, b"lvl2 user gates", b"param_set")
        _refused(lib, lib.cufhe_amd_lvl2_gate_batch(0, None, count, p, 1, out.ptr, a.ptr, a.ptr, a.ptr, W0), -1, b"param_set")
        _refused(lib, lib.cufhe_amd_lvl2_user_extract_batch(0, None, count, defs.op["one"], a.ptr, None, None, out.ptr), -1, b"param_set")
        _refused(lib, lib.cufhe_amd_lvl2_define_gate(coeffs, 0, None, ctypes.byref(got)), -1, b"param_set")
    finally:
        api.set_option("param_set", -1)
    eng.Synchronize()
    assert np.all(out.download() == FILL)


def test_cleanup_drops_the_definitions(engine2, keys, keys2, defs):
    """an op of cufhe_amd_define_gate stays refused on this ring; after cufhe_amd_cleanup the lvl2 ids are undefined, a definition
    before cufhe_amd_lvl2_initialize is refused with -3, and the first new definition is BASE + 0 again.  Runs last: it re-creates
    the engine's state for the modules that follow."""
    eng, api, lib = engine2, engine2.api, engine2.lib
    a = _upload(eng, np.zeros(2 * W0, np.uint32))
    out = api.DeviceBuffer(2 * W0).upload(np.full(2 * W0, FILL, np.uint32))
    lvl1_op = np.array([eng.define_gate((1, 1, 0), 0)], np.int32)
    rc = lib.cufhe_amd_lvl2_gate_batch(0, None, 2, lvl1_op.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, W0)
    assert rc == -1 and b"user gates run on the default path only" in lib.cufhe_amd_last_error()
    old = np.array([defs.op["one"]], np.int32)
    eng.CleanUp()
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    try:
        coeffs, got = (ctypes.c_int32 * 3)(1, 0, 0), ctypes.c_int(-7)
        _refused(lib, lib.cufhe_amd_lvl2_define_gate(coeffs, 0, None, ctypes.byref(got)), -3, b"lvl2_initialize")
        assert got.value == -7
    finally:
        eng.lvl2_initialize(keys2.bk, keys2.ksk)
    a = _upload(eng, np.zeros(2 * W0, np.uint32))
    out = api.DeviceBuffer(2 * W0).upload(np.full(2 * W0, FILL, np.uint32))
    _refused(lib, lib.cufhe_amd_lvl2_gate_batch(0, None, 2, old.ctypes.data, 0, out.ptr, a.ptr, None, None, W0), -1, b"not defined")
    _refused(lib, lib.cufhe_amd_lvl2_user_rotate_batch(0, None, 2, int(old[0]), a.ptr, None, None, 0, out.ptr), -1, b"not defined")
    api.set_option("lvl0_ring", 2048)
    try:
        _refused(lib, lib.cufhe_amd_gate_batch(0, None, 0, 2, old.ctypes.data, 0, out.ptr, a.ptr, None, None, W0), -1, b"not defined")
        c = [api.Ctxt(0) for _ in range(2)]
        _refused(lib, lib.cufhe_amd_enqueue_gate(0, None, int(old[0]), 0, c[0]._h, c[1]._h, None, None), -1, b"not defined")
    finally:
        api.set_option("lvl0_ring", 1024)
    eng.Synchronize()
    assert np.all(out.download() == FILL)
    assert eng.lvl2_define_gate((1, 0, 0), 0, defs.tv0) == eng.LVL2_USER_OP_BASE
    # the new definition runs: steps 0 of the identity input is the test vector itself
    tl = np.zeros((1, W0), np.uint32)
    dacc = api.DeviceBuffer(2 * N2 * 2)
    eng.lvl2_user_rotate_batch(eng.LVL2_USER_OP_BASE, _upload(eng, tl), dacc, 1, steps=0)
    got = dacc.download().view(np.uint64)
    assert np.all(got[:N2] == 0) and np.array_equal(got[N2:], defs.tv0)
