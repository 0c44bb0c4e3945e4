"""GPU tests of linear layers: cufhe_amd_linear_batch / _linear_list / _linear_gate_batch, word for word
against tests/linear_checker.py on random 32-bit words -- the layer is integer arithmetic mod 2^32, every input has one right answer.
The shape, footprint and capacity tests load no key.  Shapes sit on the boundaries of plan::plan_linear (tests/test_linear.py checks that plan on the
CPU): the row tile TJ, the k-unroll U, the partial last wave of a ciphertext (631 and 1025 words are no multiples of 64)."""
import ctypes
import subprocess

import numpy as np
import pytest

import footprint as fp
import linear_checker as lc
import multi_output_checker as mo
import oracle_lib as ol
import user_gate_checker as uc
from test_gpu_user_gates import MAJ, SHAPES, XOR3, set_shape

pytestmark = pytest.mark.gpu

TJ = fp.csrc_constant("kLinearRowTile", ("launch_plan.h",))
U = fp.csrc_constant("kLinearUnroll", ("launch_plan.h",))
ROWS = (1, TJ - 1, TJ, TJ + 1, 2 * TJ + 3)
COLS = (1, 2, U - 1, U + 1, 67)
SETS = (1, 3)
PAD = 9
WORDS = ol.LVL_WORDS
BASE = 20480                              # CUFHE_AMD_LINEAR_LAYER_BASE


def _restore(engine, keys):
    engine.CleanUp()
    engine.SetGPUNum(1)
    engine.Initialize(keys.bk, keys.ksk)


@pytest.fixture
def bare(engine, keys):
    """the library with a device and no key: layers need SetGPUNum only.  No layer is defined yet (CleanUp drops them)."""
    engine.CleanUp()
    engine.SetGPUNum(1)
    yield engine
    _restore(engine, keys)


@pytest.fixture
def fresh(engine, keys):
    """a freshly initialised engine: no layers and no user gates defined yet"""
    _restore(engine, keys)
    yield engine
    _restore(engine, keys)


def up(eng, arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    return eng.api.DeviceBuffer(arr.size).upload(arr)


def rows_of(flat, count, stride, words):
    """ciphertext g of a strided array: flat[g * stride : g * stride + words]"""
    return np.stack([flat[g * stride:g * stride + words] for g in range(count)]) if count else np.zeros((0, words), np.uint32)


def pointers(base, count, stride, order=None):
    order = range(count) if order is None else order
    return [base + 4 * stride * int(g) for g in order]


@pytest.mark.parametrize("level", [0, 1])
def test_shapes_on_every_tiling_boundary(bare, level):
    """rows around the row tile, cols around the k-unroll, one and three sets, packed and padded strides, with and without bias, weights
    with INT32_MIN, INT32_MAX, -1, 0 and a zero row: the batch form gives the checker's words, and the list form -- the same operands
    through pointers, the outputs in another order -- gives the same words."""
    eng, api = bare, bare.api
    words = WORDS[level]
    assert words % 64 != 0 and api.lib.cufhe_amd_ctxt_words(level) == words
    rng = np.random.default_rng(1400 + level)
    big = max(SETS) * max(COLS) * (words + PAD)
    xflat = lc.random_words(rng, big)
    din = up(eng, xflat)
    dout = api.DeviceBuffer(max(SETS) * max(ROWS) * (words + PAD))
    dlist = api.DeviceBuffer(dout.words)
    poison = np.full(dout.words, 0xDEADBEEF, np.uint32)
    failures = []
    for rows in ROWS:
        for cols in COLS:
            W = lc.test_weights(rng, rows, cols)
            bias = lc.random_words(rng, rows)
            for b in (bias, None):
                layer = eng.define_linear(W, b)
                assert (layer.rows, layer.cols) == (rows, cols)
                for sets in SETS:
                    for stride in (words, words + PAD):
                        x = rows_of(xflat, sets * cols, stride, words).reshape(sets, cols, words)
                        want = lc.linear(W, b, x).reshape(sets * rows, words)
                        dout.upload(poison)
                        eng.linear_batch(layer, level, dout, din, sets, in_stride_words=stride, out_stride_words=stride)
                        got = rows_of(dout.download(), sets * rows, stride, words)
                        order = rng.permutation(sets * rows)
                        dlist.upload(poison)
                        eng.linear_list(layer, level, pointers(dlist.ptr, sets * rows, stride, order), pointers(din.ptr, sets * cols, stride), sets)
                        listed = rows_of(dlist.download(), sets * rows, stride, words)[order]
                        if not np.array_equal(got, want) or not np.array_equal(listed, got):
                            failures.append((rows, cols, b is not None, sets, stride, int((got != want).sum()), int((listed != got).sum())))
    assert not failures, f"level {level}: (rows, cols, bias, sets, stride, wrong words batch, list != batch) {failures[:20]}"


class DeviceBackend:
    """the arena in one device allocation of the library's own allocator"""

    def __init__(self, api):
        self.api = api

    def alloc(self, words):
        self.buf = self.api.DeviceBuffer(words)
        return self.buf.ptr

    def upload(self, host):
        self.buf.upload(host)

    def download(self):
        return self.buf.download()


@pytest.mark.parametrize("form", ["batch", "list"])
@pytest.mark.parametrize("level", [0, 1])
def test_footprint(bare, level, form):
    """all operands in one allocation between patterned guards, strides larger than a ciphertext, sets 0, 1 and 3: only the `words`
    words of every output change -- the gaps between rows, the guards and the inputs stay as they were"""
    eng, api = bare, bare.api
    words = WORDS[level]
    rows, cols, stride = TJ + 1, U + 1, words + PAD
    rng = np.random.default_rng(1500 + level)
    W = lc.test_weights(rng, rows, cols)
    bias = lc.random_words(rng, rows)
    layer = eng.define_linear(W, bias)
    for sets in (0, 1, 3):
        arena = fp.Arena(f"linear_{form} level {level} sets {sets}",
                         [fp.Operand("in", np.uint32, max(sets, 1) * cols, words, "in", stride),
                          fp.Operand("out", np.uint32, max(sets, 1) * rows, words, "out", stride)], DeviceBackend(api))
        x = lc.random_words(rng, max(sets, 1) * cols, words)
        arena.set("in", x)
        if sets == 0:
            arena.written("out", [])
        arena.upload()
        if form == "batch":
            eng.linear_batch(layer, level, arena.view("out"), arena.view("in"), sets, in_stride_words=stride, out_stride_words=stride)
        else:
            eng.linear_list(layer, level, [arena.ptr("out", g) for g in range(sets * rows)], [arena.ptr("in", g) for g in range(sets * cols)], sets)
        eng.Synchronize()
        after = arena.download()
        assert arena.check(after) is None, arena.check(after)
        if sets:
            assert np.array_equal(arena.rows(after, "out"), lc.linear(W, bias, x.reshape(sets, cols, words)).reshape(sets * rows, words))


def test_refusals_leave_the_outputs_untouched(fresh, keys):
    """every refusal of the header: its status, a message, and not a word of the outputs changed"""
    eng, api, lib = fresh, fresh.api, fresh.lib
    words = WORDS[0]
    rows, cols, sets = 3, 4, 2
    rng = np.random.default_rng(1600)
    W = lc.test_weights(rng, rows, cols)
    layer = eng.define_linear(W, None)
    one = eng.define_gate((1, 0, 0), 0)
    two = eng.define_gate((1, 1, 0), 0)
    three = eng.define_gate(*MAJ)
    x = lc.random_words(rng, sets * cols, words)
    din = up(eng, x)
    poison = np.full(sets * rows * words, 0xDEADBEEF, np.uint32)
    dout = up(eng, poison)
    both = up(eng, np.concatenate([x.reshape(-1), poison]))          # in followed by out, for the overlap cases
    ins = (ctypes.c_void_p * (sets * cols))(*pointers(din.ptr, sets * cols, words))
    outs = (ctypes.c_void_p * (sets * rows))(*pointers(dout.ptr, sets * rows, words))

    def refused(rc, status, *text):
        msg = lib.cufhe_amd_last_error()
        assert rc == status and msg and all(t in msg for t in text), (rc, msg)

    def batch(layer_id=layer.id, level=0, n=sets, i=din.ptr, si=words, o=dout.ptr, so=words):
        return lib.cufhe_amd_linear_batch(0, None, layer_id, level, n, i, si, o, so)

    def fused(op=one, layer_id=layer.id, level=0, n=sets, i=din.ptr, si=words, o=dout.ptr, so=words):
        return lib.cufhe_amd_linear_gate_batch(0, None, layer_id, op, level, n, i, si, o, so)

    for call in (batch, fused):
        refused(call(i=None), -1, b"null")
        refused(call(o=None), -1, b"null")
        refused(call(layer_id=layer.id + 1), -1, b"not defined")
        refused(call(layer_id=0), -1, b"not defined")
        refused(call(level=2), -1, b"level")
        refused(call(level=-1), -1, b"level")
        refused(call(si=words - 1), -1, b"stride")
        refused(call(so=words - 1), -1, b"stride")
        # the output range begins inside the last input / ends inside the first input
        refused(call(i=both.ptr, o=both.ptr + 4 * (sets * cols * words - 1)), -1, b"overlap")
        refused(call(i=both.ptr + 4 * (sets * rows * words - 1), o=both.ptr), -1, b"overlap")
        assert call(n=0) == 0
        refused(call(level=1, si=words, so=WORDS[1]), -1, b"stride")          # a lvl0 stride under level 1
    refused(lib.cufhe_amd_linear_list(0, None, layer.id, 0, sets, None, outs), -1, b"null")
    refused(lib.cufhe_amd_linear_list(0, None, layer.id, 0, sets, ins, None), -1, b"null")
    refused(lib.cufhe_amd_linear_list(0, None, layer.id + 1, 0, sets, ins, outs), -1, b"not defined")
    refused(lib.cufhe_amd_linear_list(0, None, layer.id, 3, sets, ins, outs), -1, b"level")
    alias = (ctypes.c_void_p * (sets * rows))(*outs)
    alias[sets * rows - 1] = ins[1]
    refused(lib.cufhe_amd_linear_list(0, None, layer.id, 0, sets, ins, alias), -1, b"must not be an input")
    hole = (ctypes.c_void_p * (sets * cols))(*ins)
    hole[2] = None
    refused(lib.cufhe_amd_linear_list(0, None, layer.id, 0, sets, hole, outs), -1, b"null")
    assert lib.cufhe_amd_linear_list(0, None, layer.id, 0, 0, ins, outs) == 0
    # the fused form's own refusals: a second / third coefficient, a built-in op, ids that are no defined user gate
    refused(fused(op=two), -1, b"one operand")
    refused(fused(op=three), -1, b"one operand")
    refused(fused(op=api.NAND), -1, b"user gate")
    refused(fused(op=api.COPY), -1, b"user gate")
    refused(fused(op=three + 1), -1, b"not defined")
    refused(fused(op=api.user_op_output(one, 1)), -1, b"not an output")
    refused(fused(op=layer.id), -1, b"user gate")
    # a layer id is no op: the gate entry points refuse it by their own rule
    ops = np.array([layer.id], np.int32)
    refused(lib.cufhe_amd_gate_batch(0, None, 0, sets, ops.ctypes.data, 0, dout.ptr, din.ptr, din.ptr, None, words), -1, b"unknown gate op")
    api.set_option("lvl0_ring", 2048)
    try:
        refused(fused(), -1, b"lvl0_ring")
        din1, dout1 = api.DeviceBuffer(sets * cols * WORDS[1]), api.DeviceBuffer(sets * rows * WORDS[1])
        refused(fused(level=1, i=din1.ptr, si=WORDS[1], o=dout1.ptr, so=WORDS[1]), -1, b"lvl0_ring")
    finally:
        api.set_option("lvl0_ring", 1024)
    ps = api.ps_index("default")
    api.ps_initialize(ps, keys.bk, keys.ksk)
    api.set_option("param_set", ps)
    try:
        refused(fused(), -1, b"param_set")
        eng.Synchronize()
        assert np.array_equal(dout.download(), poison), "a refused call changed its outputs"
        # the plain layer is word arithmetic: it runs under the active set, on the set's ciphertext words
        assert lib.cufhe_amd_ctxt_words(0) == words
        eng.linear_batch(layer, 0, dout, din, sets)
        eng.Synchronize()
        assert np.array_equal(dout.download().reshape(sets * rows, words), lc.linear(W, None, x.reshape(sets, cols, words)).reshape(sets * rows, words))
        dout.upload(poison)
    finally:
        api.set_option("param_set", -1)
    eng.Synchronize()
    assert np.array_equal(dout.download(), poison), "a refused call changed its outputs"
    assert np.array_equal(din.download().reshape(x.shape), x)
    # and the same call, well formed, runs
    assert fused() == 0
    eng.Synchronize()
    assert not np.array_equal(dout.download(), poison)


def test_capacity_cleanup_and_the_fused_form_without_a_key(bare, keys):
    """64 layers, the 65th refused; without a key the plain forms run and the fused form returns -3; CleanUp drops the layers"""
    eng, api, lib = bare, bare.api, bare.lib
    words = WORDS[0]
    W = np.array([[1, -1]], np.int64)
    layers = [eng.define_linear(W, [i]) for i in range(64)]
    assert [ly.id for ly in layers] == list(range(BASE, BASE + 64))
    with pytest.raises(eng.CufheAmdError, match="full"):
        eng.define_linear(W)
    r, c = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.cufhe_amd_linear_get(layers[63].id, ctypes.byref(r), ctypes.byref(c)) == 0 and (r.value, c.value) == (1, 2)
    x = lc.random_words(np.random.default_rng(1700), 2, words)
    din, dout = up(eng, x), up(eng, np.zeros(words, np.uint32))
    eng.linear_batch(layers[63], 0, dout, din, 1)
    eng.Synchronize()
    assert np.array_equal(dout.download(), lc.linear(W, [63], x[None])[0, 0])
    rc = lib.cufhe_amd_linear_gate_batch(0, None, layers[0].id, 1000, 0, 1, din.ptr, words, dout.ptr, words)
    assert rc == -3 and b"Initialize" in lib.cufhe_amd_last_error()
    eng.CleanUp()
    eng.SetGPUNum(1)
    for ly in (layers[0], layers[63]):
        with pytest.raises(eng.CufheAmdError, match="not defined"):
            eng.linear_batch(ly, 0, dout, din, 1)
        assert lib.cufhe_amd_linear_get(ly.id, None, None) == -1
    # ids count from the base again
    assert eng.define_linear(W).id == BASE


# the fused form: (sets, rows) with sets * rows = 64, and 13 = one size above a workgroup's 8 rotations that is no multiple of 8
FUSED_SIZES = ((4, 16), (1, 13))
FUSED_COLS = 5


@pytest.mark.parametrize("kind", ["random-tv", "output-1-of-2"])
@pytest.mark.parametrize("level", [0, 1])
def test_fused_form_is_the_composition(fresh, keys, level, kind):
    """on each of the four blind-rotate launch shapes cufhe_amd_linear_gate_batch gives the words of cufhe_amd_linear_batch followed by
    cufhe_amd_gate_batch, and those are the words of linear_checker followed by the composed gate checker -- with a random test
    vector, and with output 1 of a two-output definition"""
    eng, api = fresh, fresh.api
    words = WORDS[level]
    rng = np.random.default_rng(1800 + 10 * level + len(kind))
    tv = lc.random_words(rng, ol.N)
    coeffs, off = (3, 0, 0), int(rng.integers(0, 1 << 32))
    if kind == "random-tv":
        op = eng.define_gate(coeffs, off, tv)
    else:
        op = api.user_op_output(eng.define_gate(coeffs, off, tv, nout=2), 1)
    cases = []
    for sets, rows in FUSED_SIZES:
        W = rng.integers(-4, 5, size=(rows, FUSED_COLS))
        bias = lc.random_words(rng, rows)
        x = lc.random_words(rng, sets, FUSED_COLS, words)
        sums = lc.linear(W, bias, x).reshape(sets * rows, words)
        if kind == "random-tv":
            want = uc.user_gate_batch(keys, level, coeffs, off, tv, [sums])
        else:
            want = mo.multi_gate_batch(keys, level, coeffs, off, tv, 2, [sums])[1]
        cases.append((sets, rows, eng.define_linear(W, bias), up(eng, x), want))
    try:
        for shape in SHAPES:
            set_shape(api, shape)
            for sets, rows, layer, din, want in cases:
                count = sets * rows
                dfused, dsum, dtwo = (api.DeviceBuffer(count * words) for _ in range(3))
                eng.linear_gate_batch(layer, op, level, dfused, din, sets)
                eng.linear_batch(layer, level, dsum, din, sets)
                eng.gate_batch(op, level, dtwo, dsum, count=count)
                eng.Synchronize()
                fused, two = dfused.download().reshape(count, words), dtwo.download().reshape(count, words)
                assert np.array_equal(fused, two), f"level {level} shape {shape} {sets} x {rows}: fused != linear_batch then gate_batch"
                bad = [g for g in range(count) if not np.array_equal(fused[g], want[g])]
                assert not bad, f"level {level} shape {shape} {sets} x {rows}: outputs {bad} differ from the checker"
    finally:
        set_shape(api, None)


@pytest.mark.parametrize("level", [0, 1])
def test_identity_with_the_three_input_user_gates(fresh, keys, level):
    """rows = 1, cols = 3: W = (1, 1, 1) through the one-input gate ((1, 0, 0), 0) is the three-input user gate MAJ word for word, and
    W = (2, 2, 2) with bias 4 mu is XOR3 -- both form the same x mod 2^32 -- and 64 encrypted triples decrypt to the truth tables"""
    eng, api = fresh, fresh.api
    words = WORDS[level]
    count = 64
    combos = np.array([[(c >> i) & 1 for i in range(3)] for c in range(8)], np.uint8)
    bits = np.repeat(combos, count // 8, axis=0).T                     # [3][64]
    ins = [keys.encrypt(bits[i], level, seed=1900 + 10 * level + i) for i in range(3)]
    x = np.stack(ins, axis=1)                                          # [64 sets][3 cols][words]
    din = up(eng, x)
    d3 = [up(eng, a) for a in ins]
    ident = eng.define_gate((1, 0, 0), 0)
    for (c, off), truth in ((MAJ, bits.sum(axis=0) >= 2), (XOR3, bits.sum(axis=0) % 2 == 1)):
        gate3 = eng.define_gate(c, off)
        layer = eng.define_linear(np.array([c], np.int64), [off])
        dlayer, dgate = api.DeviceBuffer(count * words), api.DeviceBuffer(count * words)
        eng.linear_gate_batch(layer, ident, level, dlayer, din, count)
        eng.gate_batch(gate3, level, dgate, d3[0], d3[1], d3[2], count=count)
        eng.Synchronize()
        got = dlayer.download().reshape(count, words)
        assert np.array_equal(got, dgate.download().reshape(count, words)), f"level {level} coefficients {c}: the layer differs from the user gate"
        assert np.array_equal(keys.decrypt(got, level), truth.astype(np.uint8)), f"level {level} coefficients {c}: truth table"


def test_cpp_linear(engine):
    """tests/cpp/test_linear.cpp: gLinear and gLinearApply on Ctxt<lvl0param> through include/cufhe_amd.hpp"""
    exe = lc.build_cpp_program()
    engine.CleanUp()                      # the C++ program owns the device state while it runs
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        k = ol.Keys(ol.load(), seed=1)
        engine.SetGPUNum(1)
        engine.Initialize(k.bk, k.ksk)
