"""GPU tests of the multi-output gates of the N = 2048 ring (cufhe_amd_lvl2_define_gate_multi) and of the one-rotation circuit
bootstrap ("cb_rotations" 1): every word comparison is equality with tests/lvl2_multi_checker.py (tied to the single-output checkers
and the oracle by tests/test_lvl2_multi_output_gates.py), on both rotation kernels of the ring.  A checker rotation costs a second or
two of CPU: every reference is computed once per module, on threads, and shared by the two kernels and by the ways a gate is called.

cufhe_amd_lvl2_gate_batch gives every row operand pointers of its own (one stride for all arrays), so rows of one call never share a
rotation there: the fusion counts are taken through cufhe_amd_gate_list and cufhe_amd_enqueue_gate with "lvl0_ring" 2048, where
siblings name the same operands."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cb_checker as cb
import footprint as fp
import lvl2_multi_checker as mc
import lvl2_user_gate_checker as lc
import oracle_lib as ol
import positions as pos
import user_gate_checker as uc
from test_gpu_circuit_bootstrap import (_loaded, _phase, _restore, _trlwe, _upload, _use, br2_kernel, engine2, keys2,  # noqa: F401
                                        random_key, random_words, real_key, real_words)
from test_gpu_footprint import DeviceBackend
from test_gpu_lvl2_user_gates import _rotate_inputs

pytestmark = pytest.mark.gpu

n, N, N2 = ol.n, ol.N, ol.N2
W0, W2 = n + 1, N2 + 1
FILL = 0xDEADBEEF
NAND, MUX = ol.OPS.index("NAND"), ol.OPS.index("MUX")
EIGHTH = 1 << 61


def _tv(seed):
    """a distinct random 64-bit word in every coefficient, with 0, 2^63 and 2^64 - 1 sown in"""
    tv = np.random.default_rng(seed).integers(0, 2**64, N2, dtype=np.uint64)
    tv[[0, 5, N2 - 1]] = [0, 1 << 63, 2**64 - 1]
    tv[[1000, 1024, 2047 - 64]] = [2**64 - 1, 0, 1 << 63]
    assert np.unique(tv[6:1000]).size == 994
    return tv


class Defs:
    """the module's definitions, from a clean table: (coeffs, offset, tv, nout) by name"""

    def __init__(self, eng):
        adder = mc.test_vector_multi([[(m & 1) * EIGHTH for m in range(4)], [(m >> 1) * EIGHTH for m in range(4)]])
        self.spec = {
            "two": ((1, -1, 2), 0xF0000001, _tv(12), 2),                     # the three-operand form
            "four": ((1, 0, 0), 0, _tv(14), 4),
            "eight": ((-1, 0, 0), 1 << 20, _tv(18), 8),                      # a negative c0 with an offset
            "single": ((3, -2, 0), 0x12345678, _tv(11), 1),
            "adder": ((1, 1, 1), 0, adder, 2),                               # sum and carry of a + b + c, p = 4
            "ident": ((1, 0, 0), 0, lc.test_vector(np.arange(4, dtype=np.uint64) * np.uint64(EIGHTH)), 1),
        }
        self.op = {}
        for k, (name, (c, off, tv, nout)) in enumerate(self.spec.items()):
            self.op[name] = eng.lvl2_define_gate(c, off, tv, nout=nout)
            assert self.op[name] == eng.LVL2_USER_OP_BASE + k

    def out(self, name, j):
        return mc.user_op_output(self.op[name], j)


@pytest.fixture(scope="module")
def defs(engine2, keys, keys2):
    _restore(engine2, keys, keys2)          # no definitions of earlier modules
    yield Defs(engine2)
    _restore(engine2, keys, keys2)          # ... and none of this one for the modules that follow


# ---- references, computed once -------------------------------------------------------------------------------------------------
_ref = {}


def _pool():
    if "pool" not in _ref:
        rng = np.random.default_rng(1860)
        _ref["pool"] = [rng.integers(0, 2**32, size=(2, W0), dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    return _ref["pool"]


def _evals(keys2, defs):
    """every output before its key switch, [nout][N2 + 1], of two / four / eight on the pool's rows 0 and 1, and of single on row 0"""
    if "evals" not in _ref:
        ins = _pool()
        jobs = [(name, r) for name in ("two", "four", "eight") for r in (0, 1)] + [("single", 0)]

        def one(k):
            name, r = jobs[k]
            c, off, tv, nout = defs.spec[name]
            return mc.multi_extract_one(keys2, c, off, tv, nout, [a[r] for a in ins])
        _ref["evals"] = dict(zip(jobs, mc.on_threads(one, len(jobs))))
    return _ref["evals"]


def _acc_reference(keys2, defs, name, steps):
    key = ("acc", name, steps)
    if key not in _ref:
        tl = _rotate_inputs(8 if steps == 0 else 4, 1870 + steps)
        c, off, tv, nout = defs.spec[name]
        _ref[key] = (tl, mc.on_threads(lambda g: mc.multi_rotate_one(keys2, c, off, tv, nout, [tl[g]], steps), tl.shape[0]))
    return _ref[key]


CB_D = 7


def _cb_inputs(keys):
    if "cb_in" not in _ref:
        tl = keys.encrypt(np.random.default_rng(1880).integers(0, 2, CB_D).astype(np.uint8), 0, seed=1881)
        tl[1, n] = 0                                             # bbar = 2 N2
        _ref["cb_in"] = tl
    return _ref["cb_in"]


def _cb_reference(keys, keys2):
    """one-rotation stage 1 of the 7 distinct inputs: [7][l][N2 + 1]"""
    if "cb" not in _ref:
        _ref["cb"] = mc.cb_rotate_batch(keys2, _cb_inputs(keys))
    return _ref["cb"]


def _profile(api, fn):
    api.profile_enable(True)
    api.profile_get(reset=True)
    try:
        fn()
        return api.profile_get(reset=True)
    finally:
        api.profile_enable(False)


# ---- accumulator words ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,steps", [("four", 0), ("four", 1), ("four", 2), ("four", 33), ("eight", 2)])
def test_accumulator_words(engine2, keys2, defs, br2_kernel, name, steps):
    """the one accumulator of a 4-output (s = 2) and an 8-output (s = 3) definition after `steps` steps; steps 0 is the gather alone
    on the 8 corner inputs, of which three have a bbar the s = 2 rounding changes"""
    tl, want = _acc_reference(keys2, defs, name, steps)
    if name == "four" and steps == 0:
        assert sum(mc.ms_bbar(int(b), 2) != mc.ms_bbar(int(b), 0) for b in tl[:5, n]) >= 3
    count = tl.shape[0]
    dacc = engine2.api.DeviceBuffer(count * 2 * N2 * 2)
    engine2.lvl2_user_rotate_batch(defs.op[name], _upload(engine2, tl), dacc, count, steps=steps)
    got = dacc.download().view(np.uint64).reshape(count, 2 * N2)
    for g in range(count):
        bad = np.flatnonzero(got[g] != want[g])
        assert bad.size == 0, f"{name}: rotation {g}: {bad.size} words differ after {steps} steps, first at {bad[:4]}"


@pytest.mark.parametrize("name", ["two", "four", "eight"])
def test_every_output_of_every_definition(engine2, keys2, defs, br2_kernel, name):
    """output j of the full rotation through cufhe_amd_lvl2_user_extract_batch == SampleExtract(j) of the checker's accumulator"""
    ev = _evals(keys2, defs)
    ar = lc.arity(defs.spec[name][0])
    d = [_upload(engine2, a) if k < ar else None for k, a in enumerate(_pool())]
    for j in range(defs.spec[name][3]):
        dt2 = engine2.api.DeviceBuffer(2 * W2 * 2)
        engine2.lvl2_user_extract_batch(defs.out(name, j), d[0], dt2, 2, in1=d[1], in2=d[2])
        got = dt2.download().view(np.uint64).reshape(2, W2)
        for r in range(2):
            assert np.array_equal(got[r], ev[(name, r)][j]), f"{name}: output {j} of evaluation {r} differs from the checker"


# ---- gates -----------------------------------------------------------------------------------------------------------------------
# (name, output j, pool row): outputs of a 2-output and a 4-output definition in scattered order, four.2 on row 0 twice, eight.5
# alone, a NAND, a MUX and a single-output user gate in between
MIX = [("four", 2, 0), ("two", 1, 0), ("NAND", 0, 0), ("four", 0, 0), ("single", 0, 0), ("two", 0, 0), ("four", 2, 0), ("MUX", 0, 1),
       ("eight", 5, 1), ("two", 1, 1), ("two", 0, 1), ("four", 1, 0)]
MIX_EVALS = len({(m, r) for m, _, r in MIX if m in ("two", "four", "eight")})          # 4 evaluations of multi-output definitions
MIX_ROTATIONS_FUSED = MIX_EVALS + 1 + 1 + 2                                            # + NAND, single, the two rotations of MUX
MIX_ROTATIONS_UNFUSED = sum(1 for m, _, _ in MIX if m in ("two", "four", "eight")) + 1 + 1 + 2


def _mix(keys2, defs):
    if "mix" not in _ref:
        ev, pool = _evals(keys2, defs), _pool()
        ops = np.array([NAND if m == "NAND" else MUX if m == "MUX" else defs.out(m, j) for m, j, _ in MIX], np.int32)
        rows = [r for _, _, r in MIX]
        ins = [np.ascontiguousarray(a[rows]) for a in pool]
        want = np.zeros((len(MIX), W0), np.uint32)
        for g, (m, j, r) in enumerate(MIX):
            if m in ("NAND", "MUX"):
                want[g] = keys2.gate_batch(ops[g:g + 1], pool[0][r:r + 1], pool[1][r:r + 1], pool[2][r:r + 1])[0]
            else:
                want[g] = keys2.keyswitch(ev[(m, r)][j])
        _ref["mix"] = dict(ops=ops, ins=ins, want=want, rows=rows)
    return _ref["mix"]


def test_mixed_lvl2_gate_batch(engine2, keys2, defs, br2_kernel):
    """every row equals the checker's words; rows of this entry point have operands of their own, so every output is an evaluation"""
    ref = _mix(keys2, defs)
    d = [_upload(engine2, a) for a in ref["ins"]]
    dout = engine2.api.DeviceBuffer(len(MIX) * W0)
    p = _profile(engine2.api, lambda: (engine2.lvl2_gate_batch(ref["ops"], dout, d[0], d[1], d[2]), engine2.Synchronize()))
    got = dout.download().reshape(len(MIX), W0)
    for g, m in enumerate(MIX):
        assert np.array_equal(got[g], ref["want"][g]), f"gate {g} {m} differs from the checker"
    assert p.blind_rotations == MIX_ROTATIONS_UNFUSED and p.keyswitches == len(MIX)


def test_mixed_list_shares_rotations_with_the_ring_selected(engine2, keys2, defs, br2_kernel):
    """the same gates on shared operands through cufhe_amd_gate_list, cufhe_amd_gate_batch and cufhe_amd_enqueue_gate with "lvl0_ring"
    2048: the same words, and one rotation per distinct evaluation, not per output"""
    eng, api = engine2, engine2.api
    ref = _mix(keys2, defs)
    api.set_option("lvl0_ring", 2048)
    try:
        dp = [_upload(eng, a) for a in _pool()]
        dout = api.DeviceBuffer(len(MIX) * W0)
        arr = lambda ps: (ctypes.c_void_p * len(MIX))(*ps)  # noqa: E731
        outs = [dout.ptr + 4 * W0 * g for g in range(len(MIX))]
        pin = [[dp[k].ptr + 4 * W0 * r for r in ref["rows"]] for k in range(3)]
        p = _profile(api, lambda: (eng.check(eng.lib.cufhe_amd_gate_list(0, None, 0, len(MIX), ref["ops"].ctypes.data, arr(outs), arr(pin[0]),
                                                                         arr(pin[1]), arr(pin[2]))), eng.Synchronize()))
        got = dout.download().reshape(len(MIX), W0)
        for g, m in enumerate(MIX):
            assert np.array_equal(got[g], ref["want"][g]), f"gate_list: gate {g} {m} differs from the checker"
        assert p.blind_rotations == MIX_ROTATIONS_FUSED and p.keyswitches == len(MIX)
        d = [_upload(eng, a) for a in ref["ins"]]
        dout2 = api.DeviceBuffer(len(MIX) * W0)
        eng.gate_batch(ref["ops"], 0, dout2, d[0], d[1], d[2], count=len(MIX))
        assert np.array_equal(dout2.download().reshape(len(MIX), W0), ref["want"]), "gate_batch differs from the checker"
        # recorded: one ciphertext per pool row and operand, so siblings name the same handles
        st = api.Stream()
        st.Create()
        cin = [[api.Ctxt(0) for _ in range(2)] for _ in range(3)]
        for k in range(3):
            for r in range(2):
                cin[k][r].tlwehost[:] = _pool()[k][r]
        cout = [api.Ctxt(0) for _ in MIX]
        for g, (m, j, r) in enumerate(MIX):
            ar = 2 if m == "NAND" else 3 if m == "MUX" else lc.arity(defs.spec[m][0])
            api.Apply(int(ref["ops"][g]), cout[g], *[cin[k][r] for k in range(ar)], st)
        api.Synchronize()
        for g, m in enumerate(MIX):
            assert np.array_equal(cout[g].tlwehost, ref["want"][g]), f"enqueue_gate: gate {g} {m} differs from the checker"
        st.Destroy()
    finally:
        api.set_option("lvl0_ring", 1024)


def test_single_output_and_builtin_ops_give_the_words_they_give_alone(engine2, keys2, defs, br2_kernel):
    ref = _mix(keys2, defs)
    d = [_upload(engine2, a) for a in ref["ins"]]
    for g, (m, _, _) in enumerate(MIX):
        if m not in ("NAND", "MUX", "single"):
            continue
        view = [fp.View(x.ptr + 4 * W0 * g, W0) for x in d]
        dout = engine2.api.DeviceBuffer(W0)
        engine2.lvl2_gate_batch(ref["ops"][g:g + 1], dout, view[0], view[1], view[2], count=1)
        assert np.array_equal(dout.download(), ref["want"][g]), f"{m} alone differs from its words in the mixed batch"


def test_full_adder_decrypts(engine2, keys, keys2, defs):
    """the worked example of INTEGRATION.md section 5.2: 64 evaluations of the p = 4, two-output table gate (sum and carry of
    a + b + c, bits as b / 8) on inputs that are themselves outputs of a gate of the ring; the sampled noise is printed"""
    rng = np.random.default_rng(1890)
    bits = rng.integers(0, 2, (3, 64))
    step = 1 << 29
    fresh = [uc.encrypt_torus(keys, 0, bits[k].astype(np.uint64) * np.uint64(step), 2.0 ** -15 * 2.0 ** 32, seed=1891 + k) for k in range(3)]
    ins = []
    for k in range(3):
        d = engine2.api.DeviceBuffer(64 * W0)
        engine2.lvl2_gate_batch(defs.op["ident"], d, _upload(engine2, fresh[k]), count=64)
        ins.append(d)
    x = bits.sum(axis=0)
    errs = []
    for j, want in ((0, x & 1), (1, x >> 1)):
        dout = engine2.api.DeviceBuffer(64 * W0)
        engine2.lvl2_gate_batch(defs.out("adder", j), dout, ins[0], ins[1], ins[2], count=64)
        ph = uc.phase(keys, 0, dout.download().reshape(64, W0)).astype(np.int64)
        assert np.array_equal(np.rint(ph / float(step)).astype(np.int64) % 8, want), f"output {j} decrypts wrongly"
        errs.append(((ph - want * step + 2**31) % 2**32 - 2**31) / 2.0 ** 32)
    errs = np.concatenate(errs)
    print(f"\nfull adder, 128 lvl0 outputs: sampled std {errs.std():.3e}, max |err| {np.abs(errs).max():.3e} "
          f"(derived sigma of a lvl0 output {lc.noise_sigmas()[1]:.3e}; half a box 1/16)")


# ---- one-rotation circuit bootstrap ------------------------------------------------------------------------------------------------
@pytest.fixture
def one_rotation(engine2):
    engine2.api.set_option("cb_rotations", 1)
    yield
    engine2.api.set_option("cb_rotations", 3)


def _cb_rotate(api, tl, count):
    d2 = api.DeviceBuffer(count * cb.CB_L * cb.PKS_IN * 2)
    api.cb_rotate_batch(_upload_words(api, tl), d2, count)
    return d2.download().view(np.uint64).reshape(count, cb.CB_L, cb.PKS_IN)


def _upload_words(api, arr):
    arr = np.ascontiguousarray(arr, np.uint32)
    return api.DeviceBuffer(arr.size).upload(arr)


def test_option_values(engine2):
    lib = engine2.lib
    try:
        for v in (0, 2, 4, -1):
            assert lib.cufhe_amd_set_option(b"cb_rotations", v) == -1 and b"cb_rotations" in lib.cufhe_amd_last_error()
        assert lib.cufhe_amd_set_option(b"cb_rotations", 1) == 0 and lib.cufhe_amd_set_option(b"cb_rotations", 3) == 0
    finally:
        engine2.api.set_option("cb_rotations", 3)


@pytest.mark.parametrize("count", [2, 5])
def test_one_rotation_stage1_words(engine2, keys, keys2, random_key, br2_kernel, count):
    """stage 1 at "cb_rotations" 1 == the checker's, `count` rotations; set back to 3 it is the three-rotation checker's again"""
    api = engine2.api
    tl, want = _cb_inputs(keys)[:count], _cb_reference(keys, keys2)[:count]
    try:
        api.set_option("cb_rotations", 1)
        res = {}
        p = _profile(api, lambda: (res.update(got=_cb_rotate(api, tl, count)), engine2.Synchronize()))
        for g in range(count):
            assert np.array_equal(res["got"][g], want[g]), f"one-rotation stage 1 of input {g} differs ({br2_kernel})"
        assert p.blind_rotations == count
    finally:
        api.set_option("cb_rotations", 3)
    res = {}
    p = _profile(api, lambda: (res.update(got=_cb_rotate(api, tl, count)), engine2.Synchronize()))
    assert p.blind_rotations == 3 * count
    if count == 2:
        if "cb3" not in _ref:
            _ref["cb3"] = cb.cb_rotate_batch(keys2, tl[1:2])
        assert np.array_equal(res["got"][1:2], _ref["cb3"]), "the default form no longer gives the three-rotation checker's words"


def test_every_row_at_every_batch_position(engine2, keys, keys2, random_key, one_rotation):
    """7 distinct inputs tiled over one launch above one rotation per CU (the quarter-wave kernel under the default rule): every row of
    every position equals its reference"""
    api = engine2.api
    count = 2 * fp.csrc_constant("kCbL") * 50 + 1          # 301 rotations: above one per CU on every MI300-class part
    got = _cb_rotate(api, pos.tile(_cb_inputs(keys), count), count)
    pos.assert_every_row(got, _cb_reference(keys, keys2), "one-rotation stage 1", groupings=(8, 256))


def test_one_rotation_composition_and_recorded(engine2, keys, keys2, random_key, one_rotation):
    """count 5 under the random private key: torus TRGSW == trgsw_from_stage1 of the one-rotation stage 1; NTT output ==
    trgsw_to_ntt_batch of the torus words; the recorded gCircuitBootstrapping == the batch result while the option is 1"""
    api = engine2.api
    count = 5
    tl = _cb_inputs(keys)[:count]
    d0 = _upload_words(api, tl)
    dt = api.DeviceBuffer(count * cb.TRGSW_WORDS)
    dn = api.DeviceBuffer(count * cb.TRGSW_WORDS * 2)
    api.circuit_bootstrap_batch(d0, count, trgsw=dt, trgsw_ntt=dn)
    torus = dt.download().reshape(count, 2 * cb.CB_L, 2, N)
    assert np.array_equal(torus, cb.trgsw_from_stage1(random_key, _cb_reference(keys, keys2)[:count])), "torus TRGSW != PrivKS of the one-rotation stage 1"
    dn2 = api.DeviceBuffer(count * cb.TRGSW_WORDS * 2)
    api.trgsw_to_ntt_batch(dt, dn2, count)
    ntt = dn.download()
    assert np.array_equal(ntt, dn2.download()), "NTT-domain output != trgsw_to_ntt_batch of the torus output"
    st = api.Stream()
    ins = [api.Ctxt(0) for _ in range(count)]
    outs = [api.TrgswNtt() for _ in range(count)]
    for g in range(count):
        ins[g].tlwehost[:] = tl[g]
        api.CircuitBootstrapping(outs[g], ins[g], st)
    api.Synchronize()
    for g in range(count):
        assert np.array_equal(outs[g].trgswhost, ntt.reshape(count, -1)[g]), f"recorded circuit bootstrap {g} != batch"


def test_one_rotation_cmux_end_to_end(engine2, keys, real_key, one_rotation):
    """64 random bits -> one-rotation circuit bootstrap -> CMUX between two known TRLWEs under the real key: every coefficient
    decrypts to the selected message with max |phase error| < 2^-3 (the condition of the three-rotation test)"""
    api = engine2.api
    count = 64
    rng = np.random.default_rng(1895)
    bits = rng.integers(0, 2, size=count).astype(np.uint8)
    tl = keys.encrypt(bits, 0, seed=1896)
    m1 = np.where(rng.integers(0, 2, size=(count, N)) == 1, 1 << 29, -(1 << 29)).astype(np.int64)
    m0 = np.where(rng.integers(0, 2, size=(count, N)) == 1, 1 << 29, -(1 << 29)).astype(np.int64)
    c1, c0 = _trlwe(api, keys.s1, m1, 13), _trlwe(api, keys.s1, m0, 14)
    dn = api.DeviceBuffer(count * cb.TRGSW_WORDS * 2)
    api.circuit_bootstrap_batch(_upload(engine2, tl), count, trgsw_ntt=dn)
    dres = api.DeviceBuffer(count * 2 * N)
    api.cmux_batch(dn, _upload(engine2, c1), _upload(engine2, c0), dres, count)
    ph = _phase(api, keys.s1, dres.download().reshape(count, 2, N))
    want = np.where(bits[:, None] == 1, m1, m0)
    err = ph - want
    sigma, mx = float(np.std(err)) / 2**32, float(np.max(np.abs(err))) / 2**32
    print(f"\none-rotation CB + 1 CMUX: phase error sigma 2^{np.log2(sigma):.2f}, max 2^{np.log2(mx):.2f} (margin 2^-3)")
    assert mx < 2.0 ** -3, "a coefficient decrypts wrongly"
    assert np.array_equal(np.sign(ph), np.sign(want))


# ---- footprint ---------------------------------------------------------------------------------------------------------------------
U32, U64, F64 = np.uint32, np.uint64, np.float64
O = fp.Operand


def _footprint(api, label, operands, fills, fn):
    arena = fp.Arena(label, operands, DeviceBackend(api))
    for name, rows in fills.items():
        arena.set(name, rows)
    arena.upload()
    fn(arena)
    api.Synchronize()
    after = arena.download()
    msg = arena.check(after)
    assert msg is None, msg
    return arena, after


@pytest.mark.parametrize("count", [0, 1, 3])
def test_footprint_of_the_one_rotation_entry_points(engine2, keys, keys2, random_key, one_rotation, br2_kernel, count):
    """cb_rotate_batch and circuit_bootstrap_batch at "cb_rotations" 1 write their documented rows and nothing else: the fourth output
    of a rotation (TVcb[4 q + 3] = 0) never reaches caller memory"""
    api = engine2.api
    tl = _cb_inputs(keys)[:count].reshape(count, W0)
    arena, after = _footprint(api, f"cb_rotate_batch x{count}", [O("in", U32, count, W0, "in"), O("tlwe2", U64, count * cb.CB_L, cb.PKS_IN, "out")],
                              {"in": tl}, lambda a: api.cb_rotate_batch(a.view("in"), a.view("tlwe2"), count))
    if count:
        assert np.array_equal(arena.rows(after, "tlwe2").reshape(count, cb.CB_L, cb.PKS_IN), _cb_reference(keys, keys2)[:count])
    _footprint(api, f"circuit_bootstrap_batch x{count}",
               [O("in", U32, count, W0, "in"), O("trgsw", U32, count, cb.TRGSW_WORDS, "out"), O("ntt", F64, count, cb.TRGSW_WORDS, "out")],
               {"in": tl}, lambda a: api.circuit_bootstrap_batch(a.view("in"), count, trgsw=a.view("trgsw"), trgsw_ntt=a.view("ntt")))


@pytest.mark.parametrize("count", [0, 1, 3])
def test_footprint_of_multi_output_gates(engine2, keys2, defs, br2_kernel, count):
    """lvl2_gate_batch with outputs of multi-output definitions and lvl2_user_extract_batch with an output id j > 0: the scratch
    outputs of the siblings nobody asked for never reach caller memory"""
    eng, api = engine2, engine2.api
    ev, pool = _evals(keys2, defs), _pool()
    picks = [("eight", 5, 1), ("four", 3, 0), ("two", 1, 1)][:count]
    ops = np.array([defs.out(m, j) for m, j, _ in picks] + [0], np.int32)
    fills = {f"in{k}": np.stack([pool[k][r] for _, _, r in picks]).reshape(count, W0) if count else np.zeros((0, W0), U32) for k in range(3)}
    operands = [O(f"in{k}", U32, count, W0, "in") for k in range(3)] + [O("out", U32, count, W0, "out")]

    def run(a):
        eng.check(eng.lib.cufhe_amd_lvl2_gate_batch(0, None, count, ops.ctypes.data, 1, a.ptr("out"), a.ptr("in0"), a.ptr("in1"), a.ptr("in2"), W0))
    arena, after = _footprint(api, f"lvl2_gate_batch x{count}", operands, fills, run)
    for g, (m, j, r) in enumerate(picks):
        assert np.array_equal(arena.rows(after, "out")[g], keys2.keyswitch(ev[(m, r)][j]))
    rows = [0, 1, 0][:count]
    fills = {"in0": pool[0][rows].reshape(count, W0)}
    arena, after = _footprint(api, f"lvl2_user_extract_batch x{count}", [O("in0", U32, count, W0, "in"), O("tlwe2", U64, count, W2, "out")], fills,
                              lambda a: eng.check(eng.lib.cufhe_amd_lvl2_user_extract_batch(0, None, count, defs.out("eight", 7), a.ptr("in0"), None,
                                                                                            None, a.ptr("tlwe2"))))
    for g, r in enumerate(rows):
        assert np.array_equal(arena.rows(after, "tlwe2")[g], ev[("eight", r)][7])


# ---- refusals, C++ -----------------------------------------------------------------------------------------------------------------
def _refused(lib, rc, status, *words):
    msg = lib.cufhe_amd_last_error()
    assert rc == status and msg and all(w in msg for w in words), (rc, msg)


def test_refusals_leave_the_output_untouched(engine2, keys, defs):
    eng, api, lib = engine2, engine2.api, engine2.lib
    count = 2
    a = _upload(eng, np.zeros(count * (N + 1), np.uint32))
    out = api.DeviceBuffer(count * W2 * 2).upload(np.full(count * W2 * 2, FILL, np.uint32))

    def batch(op, level=None):
        ops = np.array([NAND, op], np.int32)
        if level is None:
            return lib.cufhe_amd_lvl2_gate_batch(0, None, count, ops.ctypes.data, 1, out.ptr, a.ptr, a.ptr, a.ptr, W0)
        return lib.cufhe_amd_gate_batch(0, None, level, count, ops.ctypes.data, 1, out.ptr, a.ptr, a.ptr, a.ptr, W0 if level == 0 else N + 1)
    # an output id j >= nout; on a single-output definition; on an undefined slot
    _refused(lib, batch(defs.out("two", 2)), -1, b"j < nout")
    _refused(lib, batch(defs.out("four", 4)), -1, b"j < nout")
    _refused(lib, batch(defs.out("single", 1)), -1, b"j < nout")
    _refused(lib, batch(mc.user_op_output(mc.LVL2_USER_OP_BASE + 40, 1)), -1, b"j < nout")
    _refused(lib, batch(mc.LVL2_USER_OP_BASE + 40), -1, b"not defined")
    _refused(lib, lib.cufhe_amd_lvl2_user_extract_batch(0, None, count, defs.out("two", 3), a.ptr, a.ptr, a.ptr, out.ptr), -1, b"j < nout")
    _refused(lib, lib.cufhe_amd_lvl2_user_rotate_batch(0, None, count, defs.out("four", 1), a.ptr, None, None, 0, out.ptr), -1, b"output 0")
    assert batch(mc.LVL2_USER_OP_LAST + 1) == -1
    # the default ring and level 1
    _refused(lib, batch(defs.out("four", 1), level=0), -1, b"lvl2 user gates", b"2048")
    c = [api.Ctxt(0) for _ in range(4)]
    arr = (ctypes.c_void_p * 2)(c[0]._h, c[1]._h)
    api.set_option("lvl0_ring", 2048)
    try:
        _refused(lib, batch(defs.out("four", 1), level=1), -1, b"lvl2 user gates")
        _refused(lib, lib.cufhe_amd_enqueue_gate(0, None, defs.out("four", 4), 0, c[0]._h, c[1]._h, None, None), -1, b"j < nout")
        _refused(lib, lib.cufhe_amd_enqueue_gate_multi(0, None, defs.op["two"], 0, 2, arr, c[2]._h, c[3]._h, c[3]._h), -1, b"one output")
    finally:
        api.set_option("lvl0_ring", 1024)
    # definitions: nout outside {2, 4, 8}, a NULL test vector, c0 = 0
    coeffs, got = (ctypes.c_int32 * 3)(1, 1, 0), ctypes.c_int(-7)
    tv = np.zeros(N2, np.uint64)
    for nout in (0, 1, 3, 16):
        _refused(lib, lib.cufhe_amd_lvl2_define_gate_multi(coeffs, 0, nout, tv.ctypes.data, ctypes.byref(got)), -1, b"nout")
    _refused(lib, lib.cufhe_amd_lvl2_define_gate_multi(coeffs, 0, 2, None, ctypes.byref(got)), -1, b"test vector")
    _refused(lib, lib.cufhe_amd_lvl2_define_gate_multi((ctypes.c_int32 * 3)(0, 1, 0), 0, 2, tv.ctypes.data, ctypes.byref(got)), -1, b"c0")
    # "param_set" active
    ps = api.ps_index("default")
    api.ps_initialize(ps, keys.bk, keys.ksk)
    api.set_option("param_set", ps)
    try:
        _refused(lib, batch(defs.out("four", 1)), -1, b"param_set")
        _refused(lib, lib.cufhe_amd_lvl2_define_gate_multi(coeffs, 0, 2, tv.ctypes.data, ctypes.byref(got)), -1, b"param_set")
    finally:
        api.set_option("param_set", -1)
    assert got.value == -7
    eng.Synchronize()
    assert np.all(out.download() == FILL)


def test_the_65th_definition_and_cleanup(engine2, keys, keys2, defs, random_words):
    """a multi-output definition takes one of the 64 slots; after cufhe_amd_cleanup the ids are undefined and the library's own row is
    rebuilt with the next cufhe_amd_cb_initialize.  Runs last among the tests that use the module's definitions."""
    eng, api, lib = engine2, engine2.api, engine2.lib
    tv = np.zeros(N2, np.uint64)
    k = len(defs.op)
    while k < mc.LVL2_MAX_USER_GATES:
        assert eng.lvl2_define_gate((1, 1, 0), k, tv, nout=2) == mc.LVL2_USER_OP_BASE + k
        k += 1
    coeffs, got = (ctypes.c_int32 * 3)(1, 1, 0), ctypes.c_int(-7)
    _refused(lib, lib.cufhe_amd_lvl2_define_gate_multi(coeffs, 0, 2, tv.ctypes.data, ctypes.byref(got)), -1, b"full")
    assert got.value == -7
    old = defs.out("four", 1)
    _restore(eng, keys, keys2)
    a = _upload(eng, np.zeros(W0, np.uint32))
    out = api.DeviceBuffer(W2 * 2).upload(np.full(W2 * 2, FILL, np.uint32))
    _refused(lib, lib.cufhe_amd_lvl2_user_extract_batch(0, None, 1, old, a.ptr, None, None, out.ptr), -1, b"j < nout")
    _refused(lib, lib.cufhe_amd_lvl2_user_extract_batch(0, None, 1, defs.op["four"], a.ptr, None, None, out.ptr), -1, b"not defined")
    eng.Synchronize()
    assert np.all(out.download() == FILL)
    # the library's row after the cleanup: the one-rotation form runs again and a trivial input gives the test vector's own words
    _use(api, "random", random_words)
    try:
        api.set_option("cb_rotations", 1)
        tl = np.zeros((1, W0), np.uint32)                      # bbar = 2 N2, every abar 0: the accumulator stays (0, TVcb)
        got2 = _cb_rotate(api, tl, 1)[0]
    finally:
        api.set_option("cb_rotations", 3)
    for r in range(cb.CB_L):
        assert not got2[r, :N2].any() and int(got2[r, N2]) == 2 * cb.cb_mu(r), r
    # the module's definitions again, for whatever test is selected after this one
    defs.__init__(eng)


def test_cpp_both_outputs_on_streams(engine2, keys, keys2, defs):
    """tests/cpp/test_lvl2_multi_output.cpp: DefineGateLvl2(.., 2), both outputs by the per-gate API on Streams with "lvl0_ring" 2048"""
    import cpp_build
    cdefs, libs = cpp_build.hip_flags()
    root = ol.ROOT
    exe = os.path.join(root, "tests", "cpp", "test_lvl2_multi_output")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + cdefs +
                          ["-o", exe, os.path.join(root, "tests", "cpp", "test_lvl2_multi_output.cpp"),
                           "-L" + os.path.join(root, "cufhe_amd"), "-lcufhe_amd", "-L" + os.path.join(root, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(root, "cufhe_amd"), "-Wl,-rpath," + os.path.join(root, "oracle")] + libs)
    engine2.CleanUp()                      # the C++ program owns the device state while it runs
    _loaded["key"] = None
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-2000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        _restore(engine2, keys, keys2)
        defs.__init__(engine2)
