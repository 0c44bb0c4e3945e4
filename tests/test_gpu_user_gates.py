"""GPU tests of user gates (cufhe_amd_define_gate): programmable bootstrapping through a test vector read by the three default
blind-rotate kernels.  Word for word against the built-in gates (identity) and the composed checker of
tests/user_gate_checker.py (arbitrary test vectors, three-input gates), per launch shape; decrypted against truth tables;
through the per-gate API with renaming and two lanes, and through the C++ shim."""
import ctypes
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import user_gate_checker as uc

pytestmark = pytest.mark.gpu

TWO_INPUT = list(range(10))           # NAND .. ORYN
SHAPES = ["batch", "half", "ll", "ll2"]
MAJ = ((1, 1, 1), 0)
XOR3 = ((2, 2, 2), 4 * ol.MU)


@pytest.fixture
def fresh(engine, keys):
    """a freshly initialised engine: no user gates defined yet (CleanUp drops them)"""
    engine.CleanUp()
    engine.SetGPUNum(1)
    engine.Initialize(keys.bk, keys.ksk)
    yield engine
    engine.CleanUp()
    engine.SetGPUNum(1)
    engine.Initialize(keys.bk, keys.ksk)


def set_shape(api, which):
    """every launch on one blind-rotate kernel, as tests/test_gpu_parity.py forces them; None: the default rules"""
    big = 1 << 30
    if which is None:
        for k in ("ll2_threshold", "ll_threshold", "half_threshold", "ks_wg_threshold", "ks_split_threshold"):
            api.set_option(k, -1)
        return
    api.set_option("ll2_threshold", big if which == "ll2" else 0)
    api.set_option("ll_threshold", big if which == "ll" else 0)
    api.set_option("half_threshold", big if which == "half" else 0)
    api.set_option("ks_wg_threshold", 0 if which in ("batch", "half") else big)
    api.set_option("ks_split_threshold", big if which == "ll" else 0)


def gate_coeffs(L, op):
    ca, cb, om = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    L.orc_gate_coeffs(op, ctypes.byref(ca), ctypes.byref(cb), ctypes.byref(om))
    return (ca.value, cb.value, 0), (om.value * ol.MU) & 0xFFFFFFFF


def up(eng, arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    return eng.api.DeviceBuffer(arr.size).upload(arr)


def run_batch(eng, ops, level, ins, count):
    words = ol.LVL_WORDS[level]
    dins = [up(eng, a) for a in ins] + [None] * (3 - len(ins))
    dout = eng.api.DeviceBuffer(count * words)
    eng.gate_batch(ops, level, dout, dins[0], dins[1], dins[2], count=count)
    eng.Synchronize()
    return dout.download().reshape(count, words)


def random_words(rng, count, level):
    return rng.integers(0, 1 << 32, size=(count, ol.LVL_WORDS[level]), dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("level", [0, 1])
def test_identity_with_the_built_in_gates(fresh, keys, level):
    """a user gate with a built-in two-input gate's coefficients and offset, with no test vector and with an all-mu one, returns that
    gate's words: 4096 ciphertexts of all ten gates, on every launch shape"""
    eng, api = fresh, fresh.api
    count = 4096
    rng = np.random.default_rng(100 + level)
    bits = rng.integers(0, 2, size=(2, count)).astype(np.uint8)
    a, b = keys.encrypt(bits[0], level, seed=1000 + level), keys.encrypt(bits[1], level, seed=1100 + level)
    builtin = np.array([TWO_INPUT[g % 10] for g in range(count)], np.int32)
    null_ops, mu_ops = {}, {}
    for op in TWO_INPUT:
        c, off = gate_coeffs(keys.L, op)
        null_ops[op] = eng.define_gate(c, off)
        mu_ops[op] = eng.define_gate(c, off, uc.mu_test_vector())
    try:
        for shape in SHAPES:
            set_shape(api, shape)
            want = run_batch(eng, builtin, level, [a, b], count)
            for table in (null_ops, mu_ops):
                got = run_batch(eng, np.array([table[o] for o in builtin], np.int32), level, [a, b], count)
                assert np.array_equal(got, want), f"level {level} shape {shape}: user gate differs from the built-in gate"
        # and the built-in words are the oracle's (decrypt: the truth tables)
        assert np.array_equal(want[:64], keys.gate_batch(builtin[:64], level, a[:64], b[:64]))
    finally:
        set_shape(api, None)


def _random_gates(rng, k):
    """k user-gate definitions: random coefficients (one to three inputs), offsets and test vectors"""
    defs = []
    for i in range(k):
        arity = 1 + i % 3
        c = [int(rng.integers(1, 4)) * (1 if rng.integers(0, 2) else -1)]
        c += [int(rng.integers(-3, 4)) or 1 for _ in range(arity - 1)]
        c += [0] * (3 - len(c))
        tv = rng.integers(0, 1 << 32, size=ol.N, dtype=np.uint64).astype(np.uint32)
        defs.append((tuple(c), int(rng.integers(0, 1 << 32)), tv))
    return defs


@pytest.mark.parametrize("level", [0, 1])
def test_arbitrary_test_vectors_match_the_composed_checker(fresh, keys, level):
    """random test vectors, coefficients and offsets -- one-, two- and three-input gates -- on every launch shape: the words of the
    composed checker"""
    eng, api = fresh, fresh.api
    rng = np.random.default_rng(200 + level)
    defs = _random_gates(rng, 6)
    ids = [eng.define_gate(c, off, tv) for c, off, tv in defs]
    count = 24
    ins = [random_words(rng, count, level) for _ in range(3)]
    which = [g % len(defs) for g in range(count)]
    want = uc.user_gate_batch(keys, level, [defs[w][0] for w in which], [defs[w][1] for w in which],
                              [defs[w][2] for w in which], ins)
    ops = np.array([ids[w] for w in which], np.int32)
    try:
        for shape in SHAPES:
            set_shape(api, shape)
            got = run_batch(eng, ops, level, ins, count)
            bad = [g for g in range(count) if not np.array_equal(got[g], want[g])]
            assert not bad, f"level {level} shape {shape}: gates {bad} (definitions {[which[g] for g in bad]}) differ from the checker"
    finally:
        set_shape(api, None)


@pytest.mark.parametrize("level", [0, 1])
def test_mixed_list_selects_the_row_per_rotation(fresh, keys, level):
    """built-in ops and several user ops with different test vectors in one gate_list: every output is the word of that op run
    alone -- the test-vector row is chosen per rotation, in one rotation launch"""
    eng, api = fresh, fresh.api
    rng = np.random.default_rng(300 + level)
    defs = _random_gates(rng, 5)
    ids = [eng.define_gate(c, off, tv) for c, off, tv in defs]
    ids.append(eng.define_gate(*MAJ))
    menu = ids + [api.NAND, api.XOR, api.MUX, api.NOT, api.ORYN]
    count = 3 * len(menu)
    words = ol.LVL_WORDS[level]
    ins = [random_words(rng, count, level) for _ in range(3)]
    ops = np.array([menu[g % len(menu)] for g in range(count)], np.int32)
    d = [up(eng, a) for a in ins]
    dout = api.DeviceBuffer(count * words)
    ptr = lambda buf, g: buf.ptr + g * words * 4  # noqa: E731
    arr = lambda buf: (ctypes.c_void_p * count)(*[ptr(buf, g) for g in range(count)])  # noqa: E731
    eng.check(eng.lib.cufhe_amd_gate_list(0, None, level, count, ops.ctypes.data, arr(dout), arr(d[0]), arr(d[1]), arr(d[2])))
    eng.Synchronize()
    got = dout.download().reshape(count, words)
    for op in menu:
        sel = np.nonzero(ops == op)[0]
        alone = run_batch(eng, op, level, [a[sel] for a in ins], len(sel))
        assert np.array_equal(got[sel], alone), f"level {level}: op {op} in the mixed list differs from the op run alone"


@pytest.mark.parametrize("level", [0, 1])
def test_maj_and_xor3_truth_tables(fresh, keys, level):
    """MAJ = (1, 1, 1) offset 0 and XOR3 = (2, 2, 2) offset 4 mu on the mu test vector: 8 input combinations, 128 samples each"""
    eng = fresh
    maj, xor3 = eng.define_gate(*MAJ), eng.define_gate(*XOR3)
    combos = np.array([[(c >> i) & 1 for i in range(3)] for c in range(8)], np.uint8)
    bits = np.repeat(combos, 128, axis=0).T                       # [3][1024]
    count = bits.shape[1]
    ins = [keys.encrypt(bits[i], level, seed=3000 + 10 * level + i) for i in range(3)]
    for op, truth in ((maj, bits.sum(axis=0) >= 2), (xor3, bits.sum(axis=0) % 2 == 1)):
        out = run_batch(eng, op, level, ins, count)
        assert np.array_equal(keys.decrypt(out, level), truth.astype(np.uint8)), f"op {op} level {level}"


@pytest.mark.parametrize("level", [0, 1])
def test_function_on_two_bit_messages(fresh, keys, level):
    """p = 4 with a padding bit: f(m0 + m1) for two-bit inputs with m0 + m1 < 4, encrypted in numpy under the oracle's secret key;
    one bootstrap through eng.test_vector(f) decrypts to f"""
    eng = fresh
    p = 4
    f = np.array([3, 0, 2, 1])
    scale = (1 << 32) // (2 * p)
    values = (f * scale).astype(np.uint32)
    op = eng.define_gate((1, 1, 0), 0, eng.test_vector(values))
    pairs = np.array([(x, y) for x in range(4) for y in range(4) if x + y < p])
    reps = 40
    m = np.repeat(pairs, reps, axis=0)
    sigma = 2.0 ** 17 if level == 0 else 2.0 ** 9
    a = uc.encrypt_torus(keys, level, (m[:, 0] * scale).astype(np.uint64), sigma, seed=4000 + level)
    b = uc.encrypt_torus(keys, level, (m[:, 1] * scale).astype(np.uint64), sigma, seed=4100 + level)
    out = run_batch(eng, op, level, [a, b], len(m))
    ph = uc.phase(keys, level, out).astype(np.int64)
    dec = ((ph + scale // 2) // scale) % (2 * p)
    assert np.array_equal(dec, f[m.sum(axis=1)]), "decoded outputs differ from f"


def _ripple_words_batch(eng, maj, xor3, ea, eb, ec0):
    """the adders bit by bit through gate_batch: (sums [A][B][w], carry [A][w])"""
    A, B = ea.shape[0], ea.shape[1]
    c = ec0
    sums = []
    for k in range(B):
        ins = [ea[:, k], eb[:, k], c]
        sums.append(run_batch(eng, xor3, 0, ins, A))
        c = run_batch(eng, maj, 0, ins, A)
    return np.stack(sums, axis=1), c


def test_ripple_adders_through_the_per_gate_api(fresh, keys):
    """16-bit ripple-carry adders of MAJ / XOR3 user gates through cufhe_amd_enqueue_gate (one stream per adder, two bootstraps per
    bit), scheduled gate by gate on two lanes with output renaming: the sums decrypt right and the words are the batch path's"""
    eng, api = fresh, fresh.api
    maj, xor3 = eng.define_gate(*MAJ), eng.define_gate(*XOR3)
    A, B = 32, 16
    rng = np.random.default_rng(500)
    va, vb = rng.integers(0, 1 << B, A), rng.integers(0, 1 << B, A)
    abits = np.array([[(va[i] >> k) & 1 for k in range(B)] for i in range(A)], np.uint8)
    bbits = np.array([[(vb[i] >> k) & 1 for k in range(B)] for i in range(A)], np.uint8)
    ea = keys.encrypt(abits.ravel(), 0, seed=5001).reshape(A, B, -1)
    eb = keys.encrypt(bbits.ravel(), 0, seed=5002).reshape(A, B, -1)
    ec = keys.encrypt(np.zeros(A, np.uint8), 0, seed=5003)

    def ctxts(words):
        out = []
        for row in words:
            c = api.Ctxt(0)
            c.tlwehost[:] = row
            out.append(c)
        return out

    x, y = ctxts(ea.reshape(A * B, -1)), ctxts(eb.reshape(A * B, -1))
    carry = ctxts(ec)
    nxt = [api.Ctxt(0) for _ in range(A)]
    sums = [api.Ctxt(0) for _ in range(A * B)]
    sts = [api.Stream() for _ in range(A)]
    for s in sts:
        s.Create()
    api.set_option("cus_override", 24)
    api.set_option("sched_two_lane", 2)
    api.set_option("sched_rename", 1)
    try:
        api.sched_stats(reset=True)
        for k in range(B):
            for i in range(A):
                X, Y, st = x[i * B + k], y[i * B + k], sts[i]
                api.Apply(xor3, sums[i * B + k], X, Y, carry[i], st)
                api.Apply(maj, nxt[i], X, Y, carry[i], st)
                api.Apply(api.COPY, carry[i], nxt[i], st)          # in place on the carry: renaming keeps the chain one deep
        api.Synchronize()
        stats = api.sched_stats()
    finally:
        api.set_option("sched_two_lane", 1)
        api.set_option("cus_override", 0)
    assert stats.gates == 3 * A * B
    assert stats.two_lane_groups >= 1, "the flush was not scheduled on two lanes"
    got = [sum(int(keys.decrypt(sums[i * B + k].tlwehost, 0)[0]) << k for k in range(B)) +
           (int(keys.decrypt(carry[i].tlwehost, 0)[0]) << B) for i in range(A)]
    assert got == [int(va[i] + vb[i]) for i in range(A)]
    want_s, want_c = _ripple_words_batch(eng, maj, xor3, ea, eb, ec)
    assert np.array_equal(np.stack([c.tlwehost for c in sums]).reshape(A, B, -1), want_s)
    assert np.array_equal(np.stack([c.tlwehost for c in carry]), want_c)
    for s in sts:
        s.Destroy()


def test_cpp_apply_adders(engine):
    """tests/cpp/test_user_gates.cpp: DefineGate / TestVector / Apply / gApply of include/cufhe_amd.hpp (16-bit adders of MAJ / XOR3,
    a table function, lvl0 and lvl1), built like the other C++ test programs"""
    exe = uc.build_cpp_program()
    engine.CleanUp()                      # the C++ program owns the device state while it runs
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        k = ol.Keys(ol.load(), seed=1)
        engine.SetGPUNum(1)
        engine.Initialize(k.bk, k.ksk)


def test_refused_with_a_parameter_set_and_on_the_2048_ring(fresh, keys):
    """user ops exist on the default path only: with "param_set" active a definition and a user op are refused, and so is a user op
    on the N = 2048 ring ("lvl0_ring" 2048) -- status < 0 and a message, before any device work"""
    eng, api = fresh, fresh.api
    lib = eng.lib
    op = eng.define_gate(*MAJ)
    count = 4
    words0 = ol.LVL_WORDS[0]
    a = up(eng, np.zeros(count * words0, np.uint32))
    out = api.DeviceBuffer(count * words0)
    ops = np.array([op], np.int32)
    # the N = 2048 ring: refused before the path's own checks (its keys are not even loaded)
    api.set_option("lvl0_ring", 2048)
    try:
        rc = lib.cufhe_amd_gate_batch(0, None, 0, count, ops.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, words0)
        assert rc < 0 and b"user gates" in lib.cufhe_amd_last_error()
        rc = lib.cufhe_amd_lvl2_gate_batch(0, None, count, ops.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, words0)
        assert rc < 0 and b"user gates" in lib.cufhe_amd_last_error()
        c = [api.Ctxt(0) for _ in range(4)]
        rc = lib.cufhe_amd_enqueue_gate(0, None, op, 0, c[0]._h, c[1]._h, c[2]._h, c[3]._h)
        assert rc < 0 and b"user gates" in lib.cufhe_amd_last_error()
    finally:
        api.set_option("lvl0_ring", 1024)
    # a parameter set: the default set's numbers through the parameter-set kernels
    ps = api.ps_index("default")
    api.ps_initialize(ps, keys.bk, keys.ksk)
    api.set_option("param_set", ps)
    try:
        rc = lib.cufhe_amd_gate_batch(0, None, 0, count, ops.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, words0)
        assert rc < 0 and b"user gates" in lib.cufhe_amd_last_error()
        rc = lib.cufhe_amd_ps_gate_batch(ps, 0, None, count, ops.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, words0)
        assert rc < 0 and b"user gates" in lib.cufhe_amd_last_error()
        c = [api.Ctxt(0) for _ in range(4)]
        rc = lib.cufhe_amd_enqueue_gate(0, None, op, 0, c[0]._h, c[1]._h, c[2]._h, c[3]._h)
        assert rc < 0 and b"user gates" in lib.cufhe_amd_last_error()
        coeffs = (ctypes.c_int32 * 3)(1, 1, 0)
        got = ctypes.c_int(-1)
        rc = lib.cufhe_amd_define_gate(coeffs, 0, None, ctypes.byref(got))
        assert rc == -1 and b"param_set" in lib.cufhe_amd_last_error() and got.value == -1
    finally:
        api.set_option("param_set", -1)
    # the default path still runs the gate afterwards
    eng.Synchronize()
    x = keys.encrypt(np.array([1, 1, 0, 0], np.uint8), 0, seed=6001)
    y = keys.encrypt(np.array([1, 0, 1, 0], np.uint8), 0, seed=6002)
    z = keys.encrypt(np.array([0, 1, 1, 0], np.uint8), 0, seed=6003)
    assert list(keys.decrypt(run_batch(eng, op, 0, [x, y, z], 4), 0)) == [1, 1, 1, 0]


def test_capacity_and_cleanup(fresh, keys):
    """64 definitions, the 65th refused; CleanUp drops them and their ids are refused afterwards"""
    eng = fresh
    ids = [eng.define_gate((1, 1, 0), i) for i in range(eng.MAX_USER_GATES)]
    assert ids == list(range(eng.USER_OP_BASE, eng.USER_OP_BASE + eng.MAX_USER_GATES))
    with pytest.raises(eng.CufheAmdError, match="full"):
        eng.define_gate((1, 1, 0), 0)
    eng.CleanUp()
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    a = up(eng, np.zeros(2 * ol.LVL_WORDS[0], np.uint32))
    out = eng.api.DeviceBuffer(2 * ol.LVL_WORDS[0])
    with pytest.raises(eng.CufheAmdError, match="not defined"):
        eng.gate_batch(ids[0], 0, out, a, a, count=2)
