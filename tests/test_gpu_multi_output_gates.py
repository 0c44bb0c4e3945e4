"""GPU tests of multi-output user gates (cufhe_amd_define_gate_multi): 2, 4 or 8 functions of one linear combination from one blind
rotation.  Word for word against tests/multi_output_checker.py on every launch shape; fusion counted by the device profile; adders
through the per-gate API and the C++ shim; a noise sample; the refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import multi_output_checker as mc
import oracle_lib as ol
import user_gate_checker as uc
from test_gpu_user_gates import run_batch, set_shape, up

pytestmark = pytest.mark.gpu

SHAPES = ["batch", "half", "ll", "ll2"]
MU = ol.MU


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


def random_words(rng, count, level):
    return rng.integers(0, 1 << 32, size=(count, ol.LVL_WORDS[level]), dtype=np.uint64).astype(np.uint32)


def gate_list(eng, level, ops, outs, ins):
    """cufhe_amd_gate_list over device pointers: outs / ins are lists of per-gate pointers (ins: three lists)"""
    count = len(ops)
    ops = np.ascontiguousarray(ops, np.int32)
    arr = lambda ps: (ctypes.c_void_p * count)(*ps)  # noqa: E731
    eng.check(eng.lib.cufhe_amd_gate_list(0, None, level, count, ops.ctypes.data, arr(outs), arr(ins[0]), arr(ins[1]), arr(ins[2])))


def _defs(rng, eng, level):
    """one definition per (nout, arity): random coefficients, offset, test vector"""
    defs = []
    for nout in (2, 4, 8):
        for arity in (1, 2, 3):
            c = [int(rng.integers(1, 4)) * (1 if rng.integers(0, 2) else -1)] + [int(rng.integers(-3, 4)) or 1 for _ in range(arity - 1)]
            c += [0] * (3 - len(c))
            tv = rng.integers(0, 1 << 32, size=ol.N, dtype=np.uint64).astype(np.uint32)
            off = int(rng.integers(0, 1 << 32))
            defs.append(dict(c=tuple(c), off=off, tv=tv, nout=nout, op=eng.define_gate(c, off, tv, nout=nout)))
    return defs


@pytest.mark.parametrize("level", [0, 1])
def test_word_parity_with_the_checker(fresh, keys, level):
    """nout 2 / 4 / 8, arities 1 / 2 / 3: every output word of every evaluation equals the checker's, on every launch shape"""
    eng, api = fresh, fresh.api
    rng = np.random.default_rng(700 + level)
    defs = _defs(rng, eng, level)
    E = 2                                                    # evaluations per definition
    words = ol.LVL_WORDS[level]
    ins = [random_words(rng, E * len(defs), level) for _ in range(3)]
    want = {}
    from concurrent.futures import ThreadPoolExecutor
    jobs = [(di, e) for di in range(len(defs)) for e in range(E)]
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        res = list(ex.map(lambda t: mc.multi_gate_one(keys, level, defs[t[0]]["c"], defs[t[0]]["off"], defs[t[0]]["tv"], defs[t[0]]["nout"],
                                                       [a[t[0] * E + t[1]] for a in ins]), jobs))
    for t, r in zip(jobs, res):
        want[t] = r
    d = [up(eng, a) for a in ins]
    ops, outs, pin = [], [], [[], [], []]
    for di, df in enumerate(defs):
        for e in range(E):
            for j in range(df["nout"]):
                ops.append(eng.user_op_output(df["op"], j))
                for i in range(3):
                    pin[i].append(d[i].ptr + (di * E + e) * words * 4)
    dout = api.DeviceBuffer(len(ops) * words)
    outs = [dout.ptr + g * words * 4 for g in range(len(ops))]
    try:
        for shape in SHAPES:
            set_shape(api, shape)
            gate_list(eng, level, ops, outs, pin)
            eng.Synchronize()
            got = dout.download().reshape(len(ops), words)
            g = 0
            for di, df in enumerate(defs):
                for e in range(E):
                    for j in range(df["nout"]):
                        assert np.array_equal(got[g], want[(di, e)][j]), \
                            f"level {level} shape {shape}: nout {df['nout']} coeffs {df['c']} evaluation {e} output {j} differs"
                        g += 1
    finally:
        set_shape(api, None)


@pytest.mark.parametrize("level", [0, 1])
def test_mixed_list(fresh, keys, level):
    """built-in ops, single user gates and multi-output siblings in one gate_list, shuffled; a lone output j > 0, a repeated output,
    siblings on different inputs: every result equals its own reference (the op run alone / the checker)"""
    eng, api = fresh, fresh.api
    rng = np.random.default_rng(800 + level)
    words = ol.LVL_WORDS[level]
    tv4 = rng.integers(0, 1 << 32, size=ol.N, dtype=np.uint64).astype(np.uint32)
    tvs = rng.integers(0, 1 << 32, size=ol.N, dtype=np.uint64).astype(np.uint32)
    m4 = eng.define_gate((1, -2, 1), 12345, tv4, nout=4)
    single = eng.define_gate((2, 1, 0), 777, tvs)
    ins = [random_words(rng, 6, level) for _ in range(3)]
    d = [up(eng, a) for a in ins]
    P = lambda i, r: d[i].ptr + r * words * 4  # noqa: E731
    gates = []                                               # (op, input row, reference)
    ref4 = {r: mc.multi_gate_one(keys, level, (1, -2, 1), 12345, tv4, 4, [a[r] for a in ins]) for r in (0, 1, 2)}
    for j in range(4):
        gates.append((eng.user_op_output(m4, j), 0, ref4[0][j]))               # all siblings on row 0
    gates.append((eng.user_op_output(m4, 3), 1, ref4[1][3]))                   # a lone output j > 0 on row 1
    gates.append((eng.user_op_output(m4, 2), 2, ref4[2][2]))                   # row 2: output 2 twice, output 0
    gates.append((eng.user_op_output(m4, 2), 2, ref4[2][2]))
    gates.append((m4, 2, ref4[2][0]))
    for r in (3, 4):
        gates.append((single, r, uc.user_gate_one(keys, level, (2, 1, 0), 777, tvs, [ins[0][r], ins[1][r]])))
    for op in (api.NAND, api.XOR, api.MUX, api.NOT):
        gates.append((op, 5, None))
    order = rng.permutation(len(gates))
    gates = [gates[i] for i in order]
    ops = [g[0] for g in gates]
    dout = api.DeviceBuffer(len(gates) * words)
    outs = [dout.ptr + g * words * 4 for g in range(len(gates))]
    gate_list(eng, level, ops, outs, [[P(i, g[1]) for g in gates] for i in range(3)])
    eng.Synchronize()
    got = dout.download().reshape(len(gates), words)
    for k, (op, r, ref) in enumerate(gates):
        if ref is None:
            ref = run_batch(eng, op, level, [a[r:r + 1] for a in ins], 1)[0]
        assert np.array_equal(got[k], ref), f"level {level}: op {op} on row {r} differs from its reference"


def _profile(api, fn):
    api.profile_enable(True)
    api.profile_get(reset=True)
    try:
        fn()
        return api.profile_get(reset=True)
    finally:
        api.profile_enable(False)


@pytest.mark.parametrize("level", [0, 1])
def test_fusion_counts_gate_list(fresh, keys, level):
    """gate_list: one rotation per evaluation (definition, in0, in1, in2), whatever the order; level 0 key-switches every output,
    level 1 once per evaluation"""
    eng, api = fresh, fresh.api
    rng = np.random.default_rng(900 + level)
    words = ol.LVL_WORDS[level]
    tv = rng.integers(0, 1 << 32, size=ol.N, dtype=np.uint64).astype(np.uint32)
    m2 = eng.define_gate((1, 1, 1), 0, tv, nout=2)
    m8 = eng.define_gate((1, 0, 0), 0, tv, nout=8)
    R = 64
    ins = [random_words(rng, R, level) for _ in range(3)]
    d = [up(eng, a) for a in ins]
    gates = [(eng.user_op_output(m2, j), r) for r in range(R) for j in range(2)] + [(eng.user_op_output(m8, j), r) for r in range(8) for j in range(8)]
    gates = [gates[i] for i in rng.permutation(len(gates))]
    dout = api.DeviceBuffer(len(gates) * words)
    outs = [dout.ptr + g * words * 4 for g in range(len(gates))]
    pin = [[d[i].ptr + r * words * 4 for _, r in gates] for i in range(3)]
    p = _profile(api, lambda: (gate_list(eng, level, [g[0] for g in gates], outs, pin), eng.Synchronize()))
    evals = R + 8
    assert p.blind_rotations == evals
    assert p.keyswitches == (len(gates) if level == 0 else evals)


def _adder_inputs(keys, A, B, seed):
    rng = np.random.default_rng(seed)
    va, vb = rng.integers(0, 1 << B, A), rng.integers(0, 1 << B, A)
    bits = lambda v: np.array([[(int(v[i]) >> k) & 1 for k in range(B)] for i in range(A)], np.uint8)  # noqa: E731
    ab, bb = bits(va), bits(vb)
    sig = 2.0 ** 17
    ea = uc.encrypt_torus(keys, 0, (ab.ravel().astype(np.uint64) * MU), sig, seed + 1).reshape(A, B, -1)
    eb = uc.encrypt_torus(keys, 0, (bb.ravel().astype(np.uint64) * MU), sig, seed + 2).reshape(A, B, -1)
    ec = uc.encrypt_torus(keys, 0, np.zeros(A, np.uint64), sig, seed + 3)
    return va, vb, ea, eb, ec


def _adders_per_gate(eng, api, fa, ea, eb, ec, A, B):
    def ctxts(words):
        out = []
        for row in words:
            c = api.Ctxt(0)
            c.tlwehost[:] = row
            out.append(c)
        return out
    x, y = ctxts(ea.reshape(A * B, -1)), ctxts(eb.reshape(A * B, -1))
    carry = [ctxts(ec)] + [[api.Ctxt(0) for _ in range(A)] for _ in range(B)]
    sums = [api.Ctxt(0) for _ in range(A * B)]
    sts = [api.Stream() for _ in range(A)]
    for s in sts:
        s.Create()
    for k in range(B):
        for i in range(A):
            api.ApplyMulti(fa, [sums[i * B + k], carry[k + 1][i]], x[i * B + k], y[i * B + k], carry[k][i], sts[i])
    api.Synchronize()
    for s in sts:
        s.Destroy()
    return np.stack([c.tlwehost for c in sums]).reshape(A, B, -1), np.stack([c.tlwehost for c in carry[B]])


@pytest.mark.parametrize("two_lane", [0, 2])
def test_adders_through_apply_multi(fresh, keys, two_lane):
    """256 sixteen-bit adders, one 2-output gate (sum, carry) per bit through ApplyMulti: they decrypt right, their words are the batch
    path's, and they take 4096 rotations level by level and on two lanes"""
    eng, api = fresh, fresh.api
    fa = eng.define_gate((1, 1, 1), 0, mc.full_adder_tv(2), nout=2)
    A, B = 256, 16
    va, vb, ea, eb, ec = _adder_inputs(keys, A, B, 1234)
    api.set_option("sched_two_lane", two_lane)
    api.set_option("sched_rename", 1)
    if two_lane:
        api.set_option("cus_override", 24)
    try:
        api.sched_stats(reset=True)
        res = {}
        p = _profile(api, lambda: res.update(out=_adders_per_gate(eng, api, fa, ea, eb, ec, A, B)))
        stats = api.sched_stats()
    finally:
        api.set_option("sched_two_lane", 1)
        api.set_option("cus_override", 0)
    s_words, c_words = res["out"]
    assert stats.gates == 2 * A * B
    assert p.blind_rotations == A * B, f"{p.blind_rotations} rotations for {A * B} evaluations"
    assert p.keyswitches == 2 * A * B
    sbits = mc.decode(keys, 0, s_words.reshape(A * B, -1)).reshape(A, B)
    cbits = mc.decode(keys, 0, c_words)
    got = [sum(int(sbits[i, k]) << k for k in range(B)) + (int(cbits[i]) << B) for i in range(A)]
    assert got == [int(va[i] + vb[i]) for i in range(A)]
    # the batch path, bit by bit (outputs 0 and 1 as separate gates of one list: words do not depend on fusion)
    c = ec
    o0, o1 = fa, eng.user_op_output(fa, 1)
    for k in range(B):
        ins = [np.concatenate([ea[:, k], ea[:, k]]), np.concatenate([eb[:, k], eb[:, k]]), np.concatenate([c, c])]
        w = run_batch(eng, np.array([o0] * A + [o1] * A, np.int32), 0, ins, 2 * A)
        assert np.array_equal(s_words[:, k], w[:A]), f"bit {k}: sums differ from the batch path"
        c = w[A:]
    assert np.array_equal(c_words, c)


@pytest.mark.parametrize("nout", [2, 4])
def test_noise_sample(fresh, keys, nout):
    """65 536 p = 4 full adders (nout 2) / evaluations of the 4-output gate on inputs that are themselves bootstrapped outputs (the noise
    a circuit feeds a gate): zero decrypt errors"""
    eng = fresh
    K = 65536
    rng = np.random.default_rng(1000 + nout)
    ident = eng.define_gate((1, 0, 0), 0, eng.test_vector(np.array([0, MU, 2 * MU, 3 * MU], np.uint32)))
    fa = eng.define_gate((1, 1, 1), 0, mc.full_adder_tv(nout), nout=nout)
    bits = rng.integers(0, 2, size=(3, K))
    fresh_ct = [uc.encrypt_torus(keys, 0, bits[i].astype(np.uint64) * MU, 2.0 ** 17, 1100 + nout * 10 + i) for i in range(3)]
    ins = [run_batch(eng, ident, 0, [fresh_ct[i]], K) for i in range(3)]
    assert all(np.array_equal(mc.decode(keys, 0, ins[i]), bits[i]) for i in range(3))
    x = bits.sum(axis=0)
    for j in range(nout):
        out = run_batch(eng, eng.user_op_output(fa, j), 0, ins, K)
        want = (x & 1) if j % 2 == 0 else (x >> 1)
        errors = int(np.count_nonzero(mc.decode(keys, 0, out) != want))
        assert errors == 0, f"nout {nout} output {j}: {errors} decrypt errors in {K}"


def test_refusals(fresh, keys):
    """aliased outputs (nothing recorded, handles untouched), ids j >= nout, "param_set", the N = 2048 ring, ids after CleanUp"""
    eng, api = fresh, fresh.api
    lib = eng.lib
    tv = mc.full_adder_tv(2)
    m2 = eng.define_gate((1, 1, 1), 0, tv, nout=2)
    c = [api.Ctxt(0) for _ in range(5)]
    for k, ct in enumerate(c):
        ct.tlwehost[:] = k + 1
    before = [ct.tlwehost.copy() for ct in c]
    st = api.Stream()
    st.Create()
    api.sched_stats(reset=True)
    with pytest.raises(eng.CufheAmdError, match="also an input"):
        api.ApplyMulti(m2, [c[0], c[1]], c[1], c[2], c[3], st)
    with pytest.raises(eng.CufheAmdError, match="same ciphertext"):
        api.ApplyMulti(m2, [c[0], c[0]], c[2], c[3], c[4], st)
    with pytest.raises(eng.CufheAmdError, match="nout"):
        api.ApplyMulti(m2, [c[0]], c[2], c[3], c[4], st)
    api.Synchronize()
    assert api.sched_stats().gates == 0
    assert all(np.array_equal(ct.tlwehost, b) for ct, b in zip(c, before))
    st.Destroy()
    # output ids past nout, in every entry point
    words0 = ol.LVL_WORDS[0]
    a = up(eng, np.zeros(words0, np.uint32))
    out = api.DeviceBuffer(words0)
    for bad in (eng.user_op_output(m2, 2), eng.user_op_output(m2, 7), eng.user_op_output(m2 + 1, 1)):
        with pytest.raises(eng.CufheAmdError, match="unknown gate op"):
            eng.gate_batch(bad, 0, out, a, a, a, count=1)
        rc = lib.cufhe_amd_enqueue_gate(0, None, bad, 0, c[0]._h, c[2]._h, c[3]._h, c[4]._h)
        assert rc == -1 and b"unknown gate op" in lib.cufhe_amd_last_error()
    # the N = 2048 ring and a parameter set
    ops = np.array([eng.user_op_output(m2, 1)], np.int32)
    outs = (ctypes.c_void_p * 2)(c[0]._h, c[1]._h)
    api.set_option("lvl0_ring", 2048)
    try:
        rc = lib.cufhe_amd_gate_batch(0, None, 0, 1, ops.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, words0)
        assert rc < 0 and b"user gates" in lib.cufhe_amd_last_error()
        rc = lib.cufhe_amd_enqueue_gate_multi(0, None, m2, 0, 2, outs, c[2]._h, c[3]._h, c[4]._h)
        assert rc < 0 and b"user gates" in lib.cufhe_amd_last_error()
    finally:
        api.set_option("lvl0_ring", 1024)
    ps = api.ps_index("default")
    api.ps_initialize(ps, keys.bk, keys.ksk)
    api.set_option("param_set", ps)
    try:
        rc = lib.cufhe_amd_gate_batch(0, None, 0, 1, ops.ctypes.data, 0, out.ptr, a.ptr, a.ptr, a.ptr, words0)
        assert rc < 0 and b"user gates" in lib.cufhe_amd_last_error()
        rc = lib.cufhe_amd_enqueue_gate_multi(0, None, m2, 0, 2, outs, c[2]._h, c[3]._h, c[4]._h)
        assert rc < 0 and b"user gates" in lib.cufhe_amd_last_error()
        got = ctypes.c_int(-1)
        coeffs = (ctypes.c_int32 * 3)(1, 1, 1)
        rc = lib.cufhe_amd_define_gate_multi(coeffs, 0, 2, tv.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(got))
        assert rc == -1 and b"param_set" in lib.cufhe_amd_last_error() and got.value == -1
    finally:
        api.set_option("param_set", -1)
    eng.Synchronize()
    # after CleanUp the ids are gone
    eng.CleanUp()
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    for bad, msg in ((m2, "not defined"), (eng.user_op_output(m2, 1), "unknown gate op")):
        with pytest.raises(eng.CufheAmdError, match=msg):
            eng.gate_batch(bad, 0, out, a, a, a, count=1)


def build_cpp_program():
    """tests/cpp/test_multi_output_gates.cpp, with the flags tests/cpp_build.py gives the other C++ programs"""
    import cpp_build
    cdefs, libs = cpp_build.hip_flags()
    root = ol.ROOT
    exe = os.path.join(root, "tests", "cpp", "test_multi_output_gates")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + cdefs +
                          ["-o", exe, os.path.join(root, "tests", "cpp", "test_multi_output_gates.cpp"),
                           "-L" + os.path.join(root, "cufhe_amd"), "-lcufhe_amd", "-L" + os.path.join(root, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(root, "cufhe_amd"), "-Wl,-rpath," + os.path.join(root, "oracle")] + libs)
    return exe


def test_cpp_apply_multi_adders(engine):
    """tests/cpp/test_multi_output_gates.cpp: DefineGate(.., nout) / TestVectorMulti / ApplyMulti / gApplyMulti of the C++ shim"""
    exe = build_cpp_program()
    engine.CleanUp()
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        k = ol.Keys(ol.load(), seed=1)
        engine.SetGPUNum(1)
        engine.Initialize(k.bk, k.ksk)
