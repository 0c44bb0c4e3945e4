"""GPU tests of the user gates on the compiled parameter sets (cufhe_amd_ps_define_gate): every word comparison is equality with
tests/ps_user_gate_checker.py (itself tied to the set oracles by tests/test_ps_user_gates.py), on all four sets and on both launch
shapes of their blind rotation.  A reference rotation costs a fraction of a second of CPU, so the references of a set are computed once
(SetEnv caches them) and shared by the two launch shapes and by the ways a gate is called."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import footprint as fp
import oracle_lib as ol
import positions as pos
import ps_user_gate_checker as pc

pytestmark = pytest.mark.gpu

FILL = 0xDEADBEEF
MU = pc.MU
NAND, MUX = ol.OPS.index("NAND"), ol.OPS.index("MUX")
MAJ = ((1, 1, 1), 0)                 # a + b + c in {+-mu, +-3 mu}: the sign is the majority
XOR3 = ((-2, -2, -2), 0)             # -2 (a + b + c) = -+1/4 by the parity of the ones
F_TABLE = (2, 0, 3, 1)               # a non-monotone table on p = 4 messages
P = 4
# alpha0 / alpha1 of the sets (oracle/tfhe_oracle.h)
ALPHA = {"cggi16": (2.44e-5, 3.73e-9)}


def _tv(rng, N):
    """a random full-range word in every coefficient, with 0, 2^31 and 2^32 - 1 sown in"""
    tv = rng.integers(0, 2**32, N, dtype=np.uint64).astype(np.uint32)
    tv[[0, 5, N - 1]] = [0, 1 << 31, 2**32 - 1]
    tv[[N // 2, N // 2 + 1, N - 65]] = [2**32 - 1, 0, 1 << 31]
    return tv


class SetEnv:
    """one parameter set: its checker, its keys on the device, its definitions (the same ids after every setup()) and the cache of
    reference words"""

    def __init__(self, eng, base_keys, name):
        self.eng, self.api, self.lib, self.base_keys, self.name = eng, eng.api, eng.lib, base_keys, name
        self.C = pc.Checker(name, seed=5)
        self.idx = self.api.ps_index(name)
        self.cache = {}
        C, N = self.C, self.C.N
        rng = np.random.default_rng(1000 + self.idx)
        enc = lambda f: [(int(v) << 29) & 0xFFFFFFFF for v in f]  # noqa: E731
        # name -> (coeffs, offset, test vector or None, output shift); the order is the order of definition
        self.spec = {
            "one": ((1, 0, 0), 0, _tv(rng, N), 0),                       # row 0
            "row1": ((1, 0, 0), 0, _tv(rng, N), 0),                      # row 1: a row stride other than the set's N reads elsewhere
            "two": ((3, -2, 0), 0x12345678, None, 0),                    # arity 2, negative c1, an offset, TV NULL
            "three": ((1, -1, 2), 0xF0000001, _tv(rng, N), 0),           # arity 3
            "nand_null": ((-1, -1, 0), MU, None, 0),                     # NAND's (ca, cb, off) on the constant mu ...
            "nand_mu": ((-1, -1, 0), MU, C.mu_test_vector(), 0),         # ... and on the all-mu vector through the table
            "m2": ((1, 0, 0), 0, _tv(rng, N), 1),
            "m4": ((1, 1, 0), 0x01000000, _tv(rng, N), 2),
            "m8": ((1, -1, 1), 0, _tv(rng, N), 3),
            "table": ((1, 0, 0), 0, pc.test_vector(enc(F_TABLE), P, N), 0),
            "maj": (MAJ[0], MAJ[1], None, 0),
            "xor3": (XOR3[0], XOR3[1], None, 0),
            # t = ones of (a, b, c): a + b + c + 3 mu = 2 t mu sits on box 2 t of p = 4 (t >= 2: the negacyclic wrap of box 2 t - 4).
            # output 0 = carry as +-mu, output 1 = the sum bit as 0 / 2^31 (a function with f(t + 2) = -f(t))
            "adder": ((1, 1, 1), 3 * MU, pc.test_vector_multi([[-MU & 0xFFFFFFFF] * 4, [0, 0, 1 << 31, 1 << 31]], P, 2, N), 1),
        }
        self.op = {}
        self.setup()

    def setup(self):
        """the engine with nothing but the session keys, this set's keys and this set's definitions"""
        eng, api = self.eng, self.api
        eng.CleanUp()
        eng.SetGPUNum(1)
        eng.Initialize(self.base_keys.bk, self.base_keys.ksk)
        api.ps_initialize(self.idx, self.C.K.bk, self.C.K.ksk)
        for k, (name, (c, off, tv, s)) in enumerate(self.spec.items()):
            self.op[name] = api.ps_define_gate(self.idx, c, off, tv, nout=1 << s)
            assert self.op[name] == api.PS_USER_OP_BASE + k

    def ref(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def up(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint32)
        return self.api.DeviceBuffer(a.size).upload(a)

    def gate_rows(self, level, names, ins):
        """[count][words] of user gates names[g] (single-output definitions) on rows g of ins"""
        C = self.C

        def one(g):
            c, off, tv, s = self.spec[names[g]]
            arity = 3 if c[2] else 2 if c[1] else 1
            return C.user_gate_one(level, c, off, tv, [a[g] for a in ins[:arity]])[0]
        return np.stack(pc.on_threads(one, len(names)))


@pytest.fixture(scope="module", params=ol.SETS)
def env(request, engine, keys):
    e = SetEnv(engine, keys, request.param)
    yield e
    engine.CleanUp()
    engine.SetGPUNum(1)
    engine.Initialize(keys.bk, keys.ksk)


@pytest.fixture(params=["wg", "batch"])
def ps_kernel(request, engine):
    """Both launch shapes of the set's blind rotation, forced for every count: a workgroup per rotation, and a wave per rotation with
    eight rotations per workgroup."""
    engine.api.set_option("ps_batch_threshold", 1 << 30 if request.param == "wg" else 1)
    yield request.param
    engine.api.set_option("ps_batch_threshold", -1)


# ---- accumulators after 0 .. 3 steps ----
def _rotate_inputs(C, seed):
    n, nbit = C.n, C.nbit
    tl = np.random.default_rng(seed).integers(0, 2**32, size=(13, n + 1), dtype=np.uint64).astype(np.uint32)
    tl[0, :4] = 0                      # abar = 0 steps
    tl[1, n] = 0                       # bbar = 2N
    tl[2, n] = 0xFFFFFFFF              # bbar = 1 (2^s on a multi-output definition)
    tl[3, :8] = 0x7FFFFFFF
    tl[3, n] = 0x80000000              # bbar = N
    tl[4, :4] = 0xFFFFFFFF             # rounds up to 2N = 0 for every s
    for s in (0, 1, 2, 3):             # the last word that does not round up to 2N under shift s, and the first that does
        half = 1 << (32 - 2 - nbit + s)
        tl[5 + s, 0] = 2**32 - half - 1
        tl[5 + s, 1] = 2**32 - half
        tl[5 + s, 2] = half
        tl[5 + s, 3] = half - 1
    tl[9, n] = (1 << (32 - 1 - nbit)) - 1          # bbar = 2N again: just below one step of the 2N grid
    return tl


@pytest.mark.parametrize("steps", [0, 1, 2, 3])
def test_accumulator_words(env, ps_kernel, steps):
    """13 rotations (a second workgroup with idle waves in the batch shape) from row 1 of the table and from the three multi-output
    rows, the modulus switch rounded to multiples of 1, 2, 4, 8: every word of the accumulator equals the checker's"""
    C, api = env.C, env.api
    tl = _rotate_inputs(C, 300 + steps)
    # second and third operands: zero on the rows with sown words (the sum keeps them), random on the last three
    ins = [tl, np.roll(tl, 1, axis=0), np.roll(tl, 2, axis=0)]
    ins[1][:10] = 0
    ins[2][:10] = 0
    d_in = [env.up(a) for a in ins]
    for name in ("row1", "m2", "m4", "m8"):
        c, off, tv, s = env.spec[name]
        arity = 3 if c[2] else 2 if c[1] else 1
        want = env.ref(("acc", name, steps), lambda: np.stack(
            [C.user_rotate_one(c, off, tv, [a[g] for a in ins[:arity]], s, steps) for g in range(13)]))
        dacc = api.DeviceBuffer(13 * C.acc_words).upload(np.full(13 * C.acc_words, FILL, np.uint32))
        api.ps_user_rotate(env.idx, env.op[name], d_in[0], dacc, 13, in1=d_in[1] if arity >= 2 else None,
                           in2=d_in[2] if arity == 3 else None, steps=steps)
        got = dacc.download().reshape(13, -1)
        for g in range(13):
            bad = np.flatnonzero(got[g] != want[g])
            assert bad.size == 0, f"{env.name} {name}: rotation {g}: {bad.size} words differ after {steps} steps, first at {bad[:4]}"


# ---- whole gates, word for word ----
GATE_LIST = ["one", "two", "three", NAND, "nand_null", "nand_mu", MUX, "row1", "two", "three", NAND, MUX, "one"]


@pytest.mark.parametrize("level", [0, 1])
def test_whole_gates_in_one_list(env, ps_kernel, level):
    """13 gates in one list: arities 1, 2 and 3 with non-unit coefficients and an offset, test vectors NULL, all-mu and random, NAND and
    MUX mixed in -- the words of the checker; NAND's coefficients on NULL and on the all-mu vector are also orc_gate_batch's NAND"""
    C, api, K = env.C, env.api, env.C.K
    count = len(GATE_LIST)
    rng = np.random.default_rng(400 + level)
    ins = [K.encrypt(rng.integers(0, 2, count).astype(np.uint8), level, seed=410 + 3 * level + i) for i in range(3)]
    ops = np.array([g if isinstance(g, int) else env.op[g] for g in GATE_LIST], np.int32)

    def reference():
        want = np.zeros((count, C.words[level]), np.uint32)
        user = [g for g in range(count) if not isinstance(GATE_LIST[g], int)]
        rows = env.gate_rows(level, [GATE_LIST[g] for g in user], [a[user] for a in ins])
        want[user] = rows
        for g in range(count):
            if isinstance(GATE_LIST[g], int):
                want[g] = K.gate_batch(GATE_LIST[g], level, ins[0][g:g + 1], ins[1][g:g + 1], ins[2][g:g + 1])[0]
        return want
    want = env.ref(("gates", level), reference)
    dout = api.DeviceBuffer(count * C.words[level]).upload(np.full(count * C.words[level], FILL, np.uint32))
    api.ps_gate_batch(env.idx, ops, dout, env.up(ins[0]), env.up(ins[1]), env.up(ins[2]), count=count, level=level)
    got = dout.download().reshape(count, -1)
    for g in range(count):
        assert np.array_equal(got[g], want[g]), f"{env.name} level {level}: gate {g} ({GATE_LIST[g]}) differs from the checker"
    for g in (4, 5):
        nand = K.gate_batch(NAND, level, ins[0][g:g + 1], ins[1][g:g + 1])[0]
        assert np.array_equal(got[g], nand), f"{env.name} level {level}: {GATE_LIST[g]} is not the oracle's NAND"


# ---- multi-output ----
@pytest.mark.parametrize("level", [0, 1])
def test_multi_output_gates(env, ps_kernel, level):
    """nout = 2, 4, 8: all outputs in shuffled order within one list (three rotations), then only output nout - 1 of each: output j is
    SampleExtract(j) of the checker's accumulator, key switched at level 0"""
    C, api, K = env.C, env.api, env.C.K
    names = ("m2", "m4", "m8")
    ins = [K.encrypt(np.array([1], np.uint8), level, seed=500 + 3 * level + i)[0] for i in range(3)]

    def reference():
        out = {}
        rows = pc.on_threads(lambda i: C.user_gate_one(level, *env.spec[names[i]][:3], ins[:3 if env.spec[names[i]][0][2] else 2 if env.spec[names[i]][0][1] else 1],
                                                       s=env.spec[names[i]][3]), 3)
        for name, r in zip(names, rows):
            out[name] = r
        return out
    want = env.ref(("multi", level), reference)
    d = [env.up(a) for a in ins]
    words = C.words[level]
    lists = [[(name, j) for name in names for j in range(1 << env.spec[name][3])], [(name, (1 << env.spec[name][3]) - 1) for name in names]]
    np.random.default_rng(7).shuffle(lists[0])
    for wanted in lists:
        count = len(wanted)
        ops = np.array([api.ps_user_op_output(env.op[name], j) for name, j in wanted], np.int32)
        dout = api.DeviceBuffer(count * words).upload(np.full(count * words, FILL, np.uint32))
        arr = lambda b, step: (ctypes.c_void_p * count)(*[b.ptr + 4 * step * g for g in range(count)])  # noqa: E731
        # every gate of the list reads the SAME operands (outputs of one evaluation share the rotation), through cufhe_amd_gate_list
        # while "param_set" is the set
        api.set_option("param_set", env.idx)
        try:
            rc = env.lib.cufhe_amd_gate_list(0, None, level, count, ops.ctypes.data, arr(dout, words), arr(d[0], 0), arr(d[1], 0), arr(d[2], 0))
            assert rc == 0, env.lib.cufhe_amd_last_error()
            env.eng.Synchronize()
        finally:
            api.set_option("param_set", -1)
        got = dout.download().reshape(count, -1)
        for g, (name, j) in enumerate(wanted):
            assert np.array_equal(got[g], want[name][j]), f"{env.name} level {level}: output {j} of {name} ({count} gates in the list)"


# ---- decryption ----
def _sigma(name, level):
    a = ALPHA.get(name, (2.0 ** -15, 2.0 ** -25))[level]
    return a * 2.0 ** 32


@pytest.mark.parametrize("level", [0, 1])
def test_table_gate_decrypts_to_f(env, ps_kernel, level):
    """64 fresh encryptions at the set's alpha of messages on p = 4 with a padding bit, a non-monotone table through
    cufhe_amd_ps_test_vector: every output decodes to f(m)"""
    C, api = env.C, env.api
    N = C.N
    values = np.array([(v << 29) & 0xFFFFFFFF for v in F_TABLE], np.uint32)
    assert np.array_equal(api.ps_test_vector(env.idx, values), env.spec["table"][2])
    m = np.arange(64) % P
    cts = C.encrypt_torus(level, (m.astype(np.uint64) << np.uint64(29)), _sigma(env.name, level), seed=600 + level)
    dout = api.DeviceBuffer(64 * C.words[level])
    api.ps_gate_batch(env.idx, env.op["table"], dout, env.up(cts), count=64, level=level)
    ph = C.phase(level, dout.download().reshape(64, -1))
    dec = ((ph.astype(np.uint64) + np.uint64(1 << 28)) >> np.uint64(29)) % 8
    assert list(dec) == [F_TABLE[i] for i in m], f"{env.name} level {level}"
    assert N in (512, 1024)


@pytest.mark.parametrize("level", [0, 1])
def test_full_adder(env, ps_kernel, level):
    """a one-bit full adder on all eight inputs: from MAJ and XOR3, and from ONE two-output gate (carry as +-mu, the sum bit as 0 / 2^31)"""
    C, api, K = env.C, env.api, env.C.K
    combos = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)], np.uint8)
    ins = [K.encrypt(combos[:, i], level, seed=700 + 3 * level + i) for i in range(3)]
    d = [env.up(a) for a in ins]
    words = C.words[level]
    dout = api.DeviceBuffer(16 * words)
    # one list of 16 gates: MAJ and XOR3 of every input
    ops = np.array([env.op["maj"]] * 8 + [env.op["xor3"]] * 8, np.int32)
    d2 = [env.up(np.concatenate([a, a])) for a in ins]
    api.ps_gate_batch(env.idx, ops, dout, d2[0], d2[1], d2[2], count=16, level=level)
    bits = K.decrypt(dout.download().reshape(16, -1), level)
    assert list(bits[:8]) == [int(c.sum() >= 2) for c in combos], f"{env.name} level {level}: MAJ"
    assert list(bits[8:]) == [int(c.sum() & 1) for c in combos], f"{env.name} level {level}: XOR3"
    # the two-output gate: outputs 0 and 1 of each input from one rotation (cufhe_amd_gate_list on shared operand pointers)
    count = 16
    arr = lambda b, step, rep: (ctypes.c_void_p * count)(*[b.ptr + 4 * step * (g // rep) for g in range(count)])  # noqa: E731
    ops = np.array([api.ps_user_op_output(env.op["adder"], g % 2) for g in range(count)], np.int32)
    outs = (ctypes.c_void_p * count)(*[dout.ptr + 4 * words * g for g in range(count)])
    api.set_option("param_set", env.idx)
    try:
        rc = env.lib.cufhe_amd_gate_list(0, None, level, count, ops.ctypes.data, outs, arr(d[0], words, 2), arr(d[1], words, 2), arr(d[2], words, 2))
        assert rc == 0, env.lib.cufhe_amd_last_error()
        env.eng.Synchronize()
    finally:
        api.set_option("param_set", -1)
    ph = C.phase(level, dout.download().reshape(16, -1)).astype(np.int64)
    carry = [int(0 < p < 2**31) for p in ph[0::2]]
    total = [int(((p + 2**30) >> 31) & 1) for p in ph[1::2]]
    assert carry == [int(c.sum() >= 2) for c in combos], f"{env.name} level {level}: carry of the two-output adder"
    assert total == [int(c.sum() & 1) for c in combos], f"{env.name} level {level}: sum of the two-output adder"


# ---- the per-gate API ----
def test_per_gate_api_chain(env, ps_kernel):
    """with "param_set" on the set: user -> NAND -> user on two streams, one chain at each level; the words are the checker's applied
    in order, and the last result is in tlwedevices after Synchronize"""
    C, api, K, lib = env.C, env.api, env.C.K, env.lib
    api.set_option("param_set", env.idx)
    try:
        sts = [api.Stream() for _ in range(2)]
        for s in sts:
            s.Create()
        chains = []
        for level, st in zip((0, 1), sts):
            a, b, t1, t2, t3 = (api.Ctxt(level) for _ in range(5))
            ea = K.encrypt(np.array([1], np.uint8), level, seed=800 + level)[0]
            eb = K.encrypt(np.array([0], np.uint8), level, seed=810 + level)[0]
            a.tlwehost[:] = ea
            b.tlwehost[:] = eb
            api.Apply(env.op["two"], t1, a, b, st)
            api.gNand(t2, t1, t1, st)
            api.gApply(env.op["one"], t3, t2, st)
            api.CtxtCopyD2H(t3, st)
            chains.append((level, ea, eb, t1, t3, (a, b, t2)))
        api.Synchronize()
        for level, ea, eb, t1, t3, _keep in chains:
            def reference():
                w1 = env.gate_rows(level, ["two"], [ea[None, :], eb[None, :]])[0]
                w2 = K.gate_batch(NAND, level, w1[None, :], w1[None, :])[0]
                return w1, env.gate_rows(level, ["one"], [w2[None, :]])[0]
            w1, w3 = env.ref(("chain", level), reference)
            assert np.array_equal(t1.tlwehost, w1), f"{env.name} level {level}: Apply"
            assert np.array_equal(t3.tlwehost, w3), f"{env.name} level {level}: user -> NAND -> user"
            dev = np.empty(C.words[level], np.uint32)
            assert lib.cufhe_amd_memcpy_d2h(0, None, dev.ctypes.data, t3.tlwedevices[0], dev.size * 4) == 0
            assert lib.cufhe_amd_stream_synchronize(0, None) == 0
            assert np.array_equal(dev, w3), f"{env.name} level {level}: tlwedevices"
        for s in sts:
            s.Destroy()
    finally:
        api.set_option("param_set", -1)


# ---- refusals ----
def _err(lib):
    return lib.cufhe_amd_last_error()


def test_refusals(env, keys):
    """every refusal of the definitions and of the op ids: status, a message naming parameter sets, pre-filled outputs untouched"""
    api, lib, C = env.api, env.lib, env.C
    i32p = ctypes.POINTER(ctypes.c_int32)
    coeffs = (ctypes.c_int32 * 3)(1, 1, 0)
    zero = (ctypes.c_int32 * 3)(0, 1, 0)
    tv = env.spec["one"][2]
    tvp = tv.ctypes.data
    got = ctypes.c_int(-7)
    other = (env.idx + 1) % len(ol.SETS)
    op = env.op["two"]
    try:
        # definitions
        assert lib.cufhe_amd_ps_define_gate(env.idx, zero, 0, None, ctypes.byref(got)) == -1 and got.value == -7
        assert lib.cufhe_amd_ps_define_gate(env.idx, None, 0, None, ctypes.byref(got)) == -1
        assert lib.cufhe_amd_ps_define_gate(env.idx, coeffs, 0, None, None) == -1
        assert lib.cufhe_amd_ps_define_gate(len(ol.SETS), coeffs, 0, None, ctypes.byref(got)) == -1 and b"parameter set" in _err(lib)
        assert lib.cufhe_amd_ps_define_gate(-1, coeffs, 0, None, ctypes.byref(got)) == -1
        for nout in (0, 1, 3, 16):
            assert lib.cufhe_amd_ps_define_gate_multi(env.idx, coeffs, 0, nout, tvp, ctypes.byref(got)) == -1, nout
        assert lib.cufhe_amd_ps_define_gate_multi(env.idx, coeffs, 0, 2, None, ctypes.byref(got)) == -1 and got.value == -7
        assert lib.cufhe_amd_ps_define_gate(other, coeffs, 0, None, ctypes.byref(got)) == -3, "a set that is not initialised"
        assert b"parameter set" in _err(lib) and got.value == -7

        # op ids, outputs pre-filled
        count, w0 = 3, C.words[0]
        a = env.up(np.zeros(count * w0, np.uint32))
        out = api.DeviceBuffer(count * max(w0, C.words[1], ol.LVL_WORDS[1])).upload(np.full(count * max(w0, C.words[1], ol.LVL_WORDS[1]), FILL, np.uint32))
        acc = api.DeviceBuffer(count * C.acc_words).upload(np.full(count * C.acc_words, FILL, np.uint32))
        ops = np.array([op], np.int32)
        undefined = np.array([api.PS_USER_OP_BASE + len(env.spec)], np.int32)
        no_output = np.array([api.ps_user_op_output(env.op["m2"], 2)], np.int32)      # m2 has outputs 0 and 1

        def refused(rc, what):
            assert rc == -1, f"{env.name}: {what}: status {rc}"
            assert b"parameter set" in _err(lib), f"{env.name}: {what}: {_err(lib)}"

        # the default path ("param_set" off): every gate entry point
        refused(lib.cufhe_amd_gate_batch(0, None, 0, count, ops.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, ol.LVL_WORDS[0]), "default path")
        refused(lib.cufhe_amd_gate(0, None, op, 0, out.ptr, a.ptr, a.ptr, a.ptr), "default path, one gate")
        c = [api.Ctxt(0) for _ in range(4)]
        refused(lib.cufhe_amd_enqueue_gate(0, None, op, 0, c[0]._h, c[1]._h, c[2]._h, c[3]._h), "default path, enqueue_gate")
        # the N = 2048 ring
        api.set_option("lvl0_ring", 2048)
        try:
            refused(lib.cufhe_amd_gate_batch(0, None, 0, count, ops.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, ol.LVL_WORDS[0]), "N = 2048 ring")
            refused(lib.cufhe_amd_lvl2_gate_batch(0, None, count, ops.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, ol.LVL_WORDS[0]), "lvl2_gate_batch")
            refused(lib.cufhe_amd_enqueue_gate(0, None, op, 0, c[0]._h, c[1]._h, c[2]._h, c[3]._h), "N = 2048 ring, enqueue_gate")
        finally:
            api.set_option("lvl0_ring", 1024)
        # another set; an id without a definition; an output the definition lacks
        for level in (0, 1):
            refused(lib.cufhe_amd_ps_gate_batch_level(other, 0, None, level, count, ops.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, w0), "another set")
            refused(lib.cufhe_amd_ps_gate_batch_level(env.idx, 0, None, level, count, undefined.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, w0), "undefined id")
            refused(lib.cufhe_amd_ps_gate_batch_level(env.idx, 0, None, level, count, no_output.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, w0), "output 2 of 2")
        refused(lib.cufhe_amd_ps_gate_batch(other, 0, None, count, ops.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, w0), "another set")
        refused(lib.cufhe_amd_ps_user_rotate(other, 0, None, count, op, a.ptr, a.ptr, a.ptr, acc.ptr, 1), "user_rotate on another set")
        refused(lib.cufhe_amd_ps_user_rotate(env.idx, 0, None, count, int(undefined[0]), a.ptr, a.ptr, a.ptr, acc.ptr, 1), "user_rotate, undefined id")
        assert lib.cufhe_amd_ps_user_rotate(env.idx, 0, None, count, NAND, a.ptr, a.ptr, a.ptr, acc.ptr, 1) == -1
        assert lib.cufhe_amd_ps_user_rotate(env.idx, 0, None, count, api.ps_user_op_output(env.op["m2"], 1), a.ptr, None, None, acc.ptr, 1) == -1
        assert lib.cufhe_amd_ps_user_rotate(env.idx, 0, None, count, op, a.ptr, None, None, acc.ptr, 1) == -1, "a missing second operand"
        assert lib.cufhe_amd_ps_user_rotate(env.idx, 0, None, count, op, a.ptr, a.ptr, None, None, 1) == -1
        assert lib.cufhe_amd_ps_user_rotate(len(ol.SETS), 0, None, count, op, a.ptr, a.ptr, None, acc.ptr, 1) == -1
        # with the set active: the op runs through the per-gate entry points; the other id ranges and definitions stay refused
        api.set_option("param_set", env.idx)
        try:
            cs = [api.Ctxt(0) for _ in range(4)]
            refused(lib.cufhe_amd_enqueue_gate(0, None, int(undefined[0]), 0, cs[0]._h, cs[1]._h, cs[2]._h, cs[3]._h), "enqueue_gate, undefined id")
            outs = (ctypes.c_void_p * 2)(cs[0]._h, cs[1]._h)
            refused(lib.cufhe_amd_enqueue_gate_multi(0, None, env.op["m2"], 0, 2, outs, cs[2]._h, cs[3]._h, None), "enqueue_gate_multi")
            rc = lib.cufhe_amd_define_gate(coeffs, 0, None, ctypes.byref(got))
            assert rc == -1 and b"param_set" in _err(lib) and got.value == -7
            old = np.array([api.USER_OP_BASE], np.int32)
            assert lib.cufhe_amd_gate_batch(0, None, 0, count, old.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, w0) < 0
            assert lib.cufhe_amd_ps_gate_batch(env.idx, 0, None, count, old.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, w0) < 0 and b"user gates" in _err(lib)
        finally:
            api.set_option("param_set", -1)
        env.eng.Synchronize()
        assert np.all(out.download() == FILL) and np.all(acc.download() == FILL), "a refused call wrote to its output"

        # the 65th definition
        for k in range(len(env.spec), api.PS_MAX_USER_GATES):
            assert api.ps_define_gate(env.idx, (1, 1, 0), k) == api.PS_USER_OP_BASE + k
        assert lib.cufhe_amd_ps_define_gate(env.idx, coeffs, 0, None, ctypes.byref(got)) == -1 and got.value == -7
        assert lib.cufhe_amd_ps_define_gate_multi(env.idx, coeffs, 0, 2, tvp, ctypes.byref(got)) == -1 and got.value == -7
        for x in c + cs:
            x.release()
        # CleanUp drops the definitions: the id is refused afterwards, on the set it was made for
        env.eng.CleanUp()
        env.eng.SetGPUNum(1)
        env.eng.Initialize(keys.bk, keys.ksk)
        api.ps_initialize(env.idx, C.K.bk, C.K.ksk)
        refused(lib.cufhe_amd_ps_gate_batch(env.idx, 0, None, count, ops.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, w0), "after CleanUp")
        assert api.ps_define_gate(env.idx, (1, 1, 0)) == api.PS_USER_OP_BASE, "ids start again after CleanUp"
    finally:
        env.setup()


# ---- footprint ----
class DeviceBackend:
    """the arena in one device allocation of the library's own allocator (cufhe_amd_malloc)"""

    def __init__(self, api):
        self.api = api

    def alloc(self, words):
        self.buf = self.api.DeviceBuffer(words)
        return self.buf.ptr

    def upload(self, host):
        self.buf.upload(host)

    def download(self):
        return self.buf.download()


def _run_arena(env, label, operands, fills, fn):
    arena = fp.Arena(label, operands, DeviceBackend(env.api))
    try:
        for name, rows in fills.items():
            arena.set(name, rows)
        arena.upload()
        rc = fn(arena)
        sync = env.lib.cufhe_amd_synchronize()
        after = arena.download()
    finally:
        arena.backend.buf.free()
    assert rc == 0 and sync == 0, f"{label}: status {rc}, synchronize {sync}: {env.lib.cufhe_amd_last_error()}"
    msg = arena.check(after)
    assert msg is None, msg
    return arena, after


def test_footprint(env, ps_kernel):
    """cufhe_amd_ps_user_rotate (three operands, eight outputs' rounding) and cufhe_amd_ps_gate_batch with a two-output op at counts 0, 1
    and U + 1: all operands in one allocation between patterned guards, only the documented rows change"""
    C, lib = env.C, env.lib
    U = 8 if ps_kernel == "batch" else 1
    w0 = C.words[0]
    O, U32 = fp.Operand, np.uint32
    rng = np.random.default_rng(900)
    for count in (0, 1, U + 1):
        ins = [rng.integers(0, 2**32, (count, w0), dtype=np.uint64).astype(np.uint32) for _ in range(3)]
        # the accumulators of the three-operand, eight-output definition after two steps
        c, off, tv, s = env.spec["m8"]
        ops_ = [O("in0", U32, count, w0, "in"), O("in1", U32, count, w0, "in"), O("in2", U32, count, w0, "in"), O("acc", U32, count, C.acc_words, "out")]
        arena, after = _run_arena(env, f"{env.name} ps_user_rotate [{ps_kernel}], count {count}", ops_, dict(in0=ins[0], in1=ins[1], in2=ins[2]),
                                  lambda ar: lib.cufhe_amd_ps_user_rotate(env.idx, 0, None, count, env.op["m8"], ar.ptr("in0"), ar.ptr("in1"),
                                                                          ar.ptr("in2"), ar.ptr("acc"), 2))
        got = arena.rows(after, "acc")
        for g in range(count):
            assert np.array_equal(got[g], C.user_rotate_one(c, off, tv, [a[g] for a in ins], s, 2)), f"{env.name}: accumulator {g} of {count}"
        # the gate call with outputs 1, 0, 1, .. of the two-output definition: out apart from in0, then out == in0
        ops = np.array([env.api.ps_user_op_output(env.op["m2"], (g + 1) % 2) for g in range(max(count, 1))], np.int32)
        for alias in (False, True):
            if alias:
                ops_ = [O("io", U32, count, w0, "inout")]
                fills = dict(io=ins[0])
            else:
                ops_ = [O("in0", U32, count, w0, "in"), O("out", U32, count, w0, "out")]
                fills = dict(in0=ins[0])
            arena, after = _run_arena(env, f"{env.name} ps_gate_batch [{ps_kernel}{', out == in0' if alias else ''}], count {count}", ops_, fills,
                                      lambda ar: lib.cufhe_amd_ps_gate_batch(env.idx, 0, None, count, ops.ctypes.data, 1, ar.ptr("io" if alias else "out"),
                                                                             ar.ptr("io" if alias else "in0"), None, None, w0))
            got = arena.rows(after, "io" if alias else "out")
            if alias:
                assert not np.any((got == ins[0]).all(axis=1)), f"{env.name}: a row of {count} was not written"
            else:
                assert not np.any((got == pos.POISON).all(axis=1)), f"{env.name}: a row of {count} was not written"


# ---- C++ ----
def test_cpp_program_on_the_k2n512_set(engine, keys):
    """tests/cpp/test_ps_user_gates.cpp built with -DCUFHE_AMD_PARAM_SET_K2N512: DefineGate / TestVector / Apply of include/cufhe_amd.hpp
    on Ctxt<lvl0param> and Ctxt<lvl1param> while Initialize has put the per-gate API on a compiled set"""
    exe = pc.build_cpp_program()
    engine.CleanUp()
    try:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "ALL PASS" in r.stdout, r.stdout[-2000:]
    finally:
        engine.SetGPUNum(1)
        engine.Initialize(keys.bk, keys.ksk)
