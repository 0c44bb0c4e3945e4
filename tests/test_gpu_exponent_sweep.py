"""GPU sweep of the exponent axis: every rotation exponent, at both ends of its rounding interval, through every kernel that turns
ciphertext words into X^bbar or X^abar.  One launch carries all exponents: row g holds exponent index g // 2 at edge g % 2 (one more
row of random words makes the count odd), every other word random, and every word of every row is compared.

    bbar, 0 steps    the launch is the kernel's prologue; the reference is tests/exponent_sweep.py alone (start_acc)
    abar, 1 step     set through word 0 with bbar = 2N, from random content (a caller's table on the default ring, a random test-vector
                     row on the N = 2048 ring and the parameter sets); the reference is exponent_sweep's rotation and the oracle's CMux
                     (orc_cmux; on the ring the composed step of tests/lvl2_user_gate_checker.py); and from the constant mu through the
                     built-in rotations against orc_blind_rotate / orc2_blind_rotate, whose rounding is code of its own
    TRLWE level      trlwe_rotate_batch / cmux_rotate_batch with all 2N exponents, sample_extract_index_batch with all N indices,
                     and outputs 1 .. 7 of an eight-output lookup against extract() of the rotation hook's accumulator

The default ring has no accumulator hook for user gates, so their prologue is observed through whole level-0 gates whose mask words
all switch to abar = 0: such a CMux step decomposes X^0 acc - acc = 0 into zero digits and adds nothing, the rotation returns its
first accumulator, and the gate is KeySwitch(SampleExtract(j)(start_acc)) -- coefficient j of X^bbar TV for every bbar.  The full
accumulator of the same gather (rotated_tv_coef) is swept through the table path.

tests/test_exponent_sweep.py pins the reference against every other checker of tests/ first.  References are computed once per
module and shared by the launch shapes."""
import numpy as np
import pytest

import exponent_sweep as es
import lut_checker as lc
import lvl2_multi_checker as m2
import lvl2_user_gate_checker as l2
import oracle_lib as ol
import packed_rom_checker as pr
import ps_user_gate_checker as pc
import user_gate_checker as uc
from test_gpu_circuit_bootstrap import _loaded, _upload, br2_kernel, engine2, keys2  # noqa: F401
from test_gpu_packed_rom import to_ntt
from test_gpu_user_gates import run_batch, set_shape, up

pytestmark = pytest.mark.gpu

n, N, N2 = ol.n, ol.N, ol.N2
SHAPES = ["batch", "half", "ll", "ll2"]
SHIFTS = (0, 1, 2, 3)
FILL = 0xA5A5A5A5
TABLES = 5
_ref = {}


def once(key, make):
    if key not in _ref:
        _ref[key] = make()
    return _ref[key]


def words32(rng, *shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


def same(got, want, edges, which, what):
    msg = es.describe(got, want, edges, which)
    assert msg is None, "%s: %s" % (what, msg)


def with_offset(rows, off):
    """the operand a gate with offset `off` must be given for its linear part to be `rows`"""
    x = rows.copy()
    x[:, -1] = (rows[:, -1].astype(np.int64) - off) & es.M32
    return x


def force(api, shape):
    """set_shape, and no cut of a launch above one grid round into full rounds on the batch kernel plus a tail: with the cut only
    the tail of these 4097-rotation launches would run on the forced kernel.  None: the default rules again"""
    set_shape(api, shape)
    api.set_option("tail_split", 1 if shape is None else 0)


def bbar_identity(rows, nbit, s):
    """every row but the extra one gets a random last word of the first interval: bbar = 2N"""
    rows[:-1, -1] &= np.uint32((1 << (31 - nbit + s)) - 1)
    return rows


@pytest.fixture(scope="module", autouse=True)
def tidy(engine, keys):
    """a clean engine before the module's definitions and after them"""
    def clean():
        engine.CleanUp()
        _loaded["key"] = None             # test_gpu_circuit_bootstrap's note of the private key-switching key: CleanUp dropped it
        engine.SetGPUNum(1)
        engine.Initialize(keys.bk, keys.ksk)
    clean()
    yield
    clean()


# ---- the default ring ------------------------------------------------------------------------------------------------------------
class Ring1:
    """edges, rows and tables of the default ring, and its four user gates (2^s outputs, a random row and a random offset each)"""

    def __init__(self, engine):
        rng = np.random.default_rng(2600)
        self.E = {s: es.edge_words(10, s) for s in SHIFTS}
        self.b_rows = {s: es.sweep_rows(self.E[s], "b", n, rng) for s in SHIFTS}
        self.a_rows = {s: bbar_identity(es.sweep_rows(self.E[s], "a", n, rng), 10, s) for s in SHIFTS}
        self.tables = words32(rng, TABLES, 2 * N)
        self.src = {s: (np.arange(self.b_rows[s].shape[0]) * 3 + 1) % TABLES for s in SHIFTS}
        self.tv = {s: words32(rng, N) for s in SHIFTS}
        self.off = {s: int(rng.integers(1, 1 << 32)) for s in SHIFTS}
        self.op = {s: engine.api.define_gate((1, 0, 0), self.off[s], self.tv[s], nout=1 << s) for s in SHIFTS}
        # operands of the whole gates: the swept last word, mask words that all switch to abar = 0 under the gate's shift
        self.gate_in = {}
        for s in SHIFTS:
            x = with_offset(self.b_rows[s], self.off[s])
            half = 1 << (20 + s)
            x[:, :n] = ((rng.integers(0, 2 * half, size=(x.shape[0], n)) - half) & es.M32).astype(np.uint32)
            assert all(es.ms_abar(a, 10, s) == 0 for a in x[::97, :n].ravel()[::13])
            self.gate_in[s] = x


@pytest.fixture(scope="module")
def ring1(engine, tidy):
    return Ring1(engine)


def lut_rotate(engine, x, tables, src, nout, steps):
    count = x.shape[0]
    dacc = up(engine, np.full(count * 2 * N, FILL, np.uint32))
    engine.api.lut_rotate_batch(up(engine, x), up(engine, tables), dacc, count, tables.shape[0], src=src, nout=nout, steps=steps)
    engine.Synchronize()
    return dacc.download().reshape(count, 2 * N)


@pytest.mark.parametrize("shape", SHAPES)
def test_bbar_of_the_built_in_rotation(engine, ring1, shape):
    """blind_rotate_batch, 0 steps: (0, X^bbar mu) at both edge words of all 2N values of bbar (4097 rotations: an odd count, so the
    last workgroup of the paired kernel holds one rotation)"""
    rows, E = ring1.b_rows[0], ring1.E[0]
    want = once("mu1", lambda: np.stack([es.start_acc("mu", b, 0, 10) for b in rows[:, n]]))
    force(engine.api, shape)
    try:
        dacc = up(engine, np.full(rows.shape[0] * 2 * N, FILL, np.uint32))
        engine.api.blind_rotate_batch(up(engine, rows), dacc, rows.shape[0], 0)
        engine.Synchronize()
        same(dacc.download(), want, E, "b", "built-in mu on " + shape)
    finally:
        force(engine.api, None)


@pytest.mark.parametrize("shape", SHAPES)
def test_bbar_of_a_callers_table(engine, ring1, shape):
    """lut_rotate_batch, 0 steps, nout 1, 2, 4, 8: X^bbar (A, B) of random tables, both polynomials, on the grid of every shift"""
    force(engine.api, shape)
    try:
        for s in SHIFTS:
            rows, E, src = ring1.b_rows[s], ring1.E[s], ring1.src[s]
            want = once(("table", s), lambda: np.stack([es.start_acc("table", rows[g, n], s, 10, table=ring1.tables[src[g]])
                                                        for g in range(rows.shape[0])]))
            same(lut_rotate(engine, rows, ring1.tables, src, 1 << s, 0), want, E, "b", "table, nout %d on %s" % (1 << s, shape))
    finally:
        force(engine.api, None)


def gate_reference(keys, ring1, s):
    rows, tv = ring1.b_rows[s], ring1.tv[s]

    def one(g):
        acc = es.start_acc("tv", rows[g, n], s, 10, tv=tv)
        return np.stack([keys.keyswitch(es.extract(acc, j, N)) for j in range(1 << s)])
    return np.stack(lc.on_threads(one, rows.shape[0]))


@pytest.mark.parametrize("s", SHIFTS)
def test_bbar_of_user_gates(engine, keys, ring1, s):
    """a single-output user gate (s = 0) and multi-output definitions (s = 1, 2, 3) with random rows, all four shapes: every output of
    every gate is the key switch of SampleExtract(j) of (0, X^bbar TV) -- see the module's note on abar = 0"""
    api = engine.api
    rows, E, nout = ring1.b_rows[s], ring1.E[s], 1 << s
    want = once(("gate", s), lambda: gate_reference(keys, ring1, s))
    x = np.repeat(ring1.gate_in[s], nout, axis=0)
    ops = np.tile(np.array([api.user_op_output(ring1.op[s], j) if nout > 1 else ring1.op[s] for j in range(nout)], np.int32), rows.shape[0])
    try:
        for shape in SHAPES:
            force(api, shape)
            got = run_batch(engine, ops, 0, [x], x.shape[0])
            same(got.reshape(rows.shape[0], -1), want, E, "b", "user gate, %d outputs on %s" % (nout, shape))
    finally:
        force(api, None)


def table_step_reference(keys, ring1, s):
    rows, src = ring1.a_rows[s], ring1.src[s]
    bk0 = np.ascontiguousarray(keys.bk[:uc.STEP_WORDS])

    def one(g):
        acc = es.start_acc("table", rows[g, n], s, 10, table=ring1.tables[src[g]])
        rot = es.rotate_many(acc.reshape(2, N), es.ms_abar(rows[g, 0], 10, s), N).reshape(-1)
        res = np.empty(2 * N, np.uint32)
        keys.L.orc_cmux(res, bk0, rot, acc)
        return res
    return np.stack(lc.on_threads(one, rows.shape[0]))


@pytest.mark.parametrize("shape", SHAPES)
def test_abar_of_the_first_step(engine, keys, ring1, shape):
    """lut_rotate_batch, 1 step from random tables left in place (bbar = 2N): both edge words of all 2N values of abar, and the coarse
    grid of a four-output rotation (s = 2)"""
    force(engine.api, shape)
    try:
        for s in (0, 2):
            rows, E = ring1.a_rows[s], ring1.E[s]
            assert all(es.ms_bbar(b, 10, s) == 2 * N for b in rows[:-1:41, n])
            want = once(("step", s), lambda: table_step_reference(keys, ring1, s))
            same(lut_rotate(engine, rows, ring1.tables, ring1.src[s], 1 << s, 1), want, E, "a", "one step, nout %d on %s" % (1 << s, shape))
    finally:
        force(engine.api, None)


@pytest.mark.parametrize("shape", SHAPES)
def test_abar_of_the_built_in_first_step(engine, keys, ring1, shape):
    """blind_rotate_batch, 1 step: the kernels' own rounding of the mask words (not the table prologue's) against orc_blind_rotate.
    The start is the constant mu (bbar = 2N), and X^abar mu has a different sign pattern for each of the 2N values of abar"""
    rows, E = ring1.a_rows[0], ring1.E[0]
    want = once("mu1 step", lambda: np.stack(lc.on_threads(lambda g: keys.blind_rotate(rows[g], 1), rows.shape[0])))
    force(engine.api, shape)
    try:
        dacc = up(engine, np.full(rows.shape[0] * 2 * N, FILL, np.uint32))
        engine.api.blind_rotate_batch(up(engine, rows), dacc, rows.shape[0], 1)
        engine.Synchronize()
        same(dacc.download(), want, E, "a", "built-in mu, one step on " + shape)
    finally:
        force(engine.api, None)


# ---- TRLWE-level kernels ----------------------------------------------------------------------------------------------------------
def test_trlwe_rotation_by_every_exponent(engine):
    rng = np.random.default_rng(2700)
    c = words32(rng, 2 * N, 2 * N)
    e = rng.permutation(2 * N).astype(np.int32)
    dout = up(engine, np.full(c.size, FILL, np.uint32))
    engine.api.trlwe_rotate_batch(up(engine, c), e, dout, 2 * N)
    engine.Synchronize()
    got = dout.download().reshape(2 * N, -1)
    want = np.stack([es.rotate_many(c[g].reshape(2, N), int(e[g]), N).reshape(-1) for g in range(2 * N)])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%d rows differ, first exponent %d" % (bad.size, e[bad[0]])


def test_rotating_cmux_by_every_exponent(engine, keys):
    """cmux_rotate_batch out of place under a selector of bit 1: c + TRGSW [x] (X^e c - c) for all 2N exponents"""
    rng = np.random.default_rng(2701)
    c = words32(rng, 2 * N, 2 * N)
    e = rng.permutation(2 * N).astype(np.int32)
    trgsw = pr.selector(keys, 1)

    def one(g):
        res = np.empty(2 * N, np.uint32)
        keys.L.orc_cmux(res, trgsw, es.rotate_many(c[g].reshape(2, N), int(e[g]), N).reshape(-1), c[g])
        return res
    want = np.stack(lc.on_threads(one, 2 * N))
    dc, dres = up(engine, c), up(engine, np.full(c.size, FILL, np.uint32))
    engine.api.cmux_rotate_batch(to_ntt(engine, trgsw), e, dc, dres, 2 * N)
    engine.Synchronize()
    got = dres.download().reshape(2 * N, -1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%d rows differ, first exponent %d" % (bad.size, e[bad[0]])
    assert np.array_equal(dc.download().reshape(2 * N, -1), c)


def test_extraction_at_every_index(engine):
    rng = np.random.default_rng(2702)
    c = words32(rng, 7, 2 * N)
    idx = rng.permutation(N).astype(np.int32)
    src = (np.arange(N) % 7).astype(np.int32)
    d1 = up(engine, np.full(N * (N + 1), FILL, np.uint32))
    engine.api.sample_extract_index_batch(up(engine, c), idx, d1, N, src=src)
    engine.Synchronize()
    got = d1.download().reshape(N, N + 1)
    want = np.stack([es.extract(c[src[g]], int(idx[g]), N) for g in range(N)])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "%d rows differ, first index %d" % (bad.size, idx[bad[0]])


@pytest.mark.parametrize("shape", SHAPES)
def test_outputs_of_an_eight_output_lookup(engine, keys, ring1, shape):
    """lut_lookup_batch with nout = 8 (extract_more behind output 0): output j is the key switch of extract(acc, j) of the accumulator
    that lut_rotate_batch returns for the same rotation, a full one from random tables (both polynomials non-zero)"""
    api = engine.api
    count = 9
    x, src = ring1.b_rows[3][100:100 + count], ring1.src[3][:count]
    force(api, shape)
    try:
        acc = lut_rotate(engine, x, ring1.tables, src, 8, -1)
        dout = up(engine, np.full(count * 8 * (n + 1), FILL, np.uint32))
        api.lut_lookup_batch(up(engine, x), up(engine, ring1.tables), dout, count, TABLES, src=src, nout=8)
        engine.Synchronize()
        got = dout.download().reshape(count, 8, n + 1)
    finally:
        force(api, None)
    want = np.stack(lc.on_threads(lambda i: keys.keyswitch(es.extract(acc[i // 8], i % 8, N)), count * 8)).reshape(count, 8, n + 1)
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, "%s: %d outputs differ, first (rotation, output) %s" % (shape, len(bad), tuple(bad[0]))


# ---- the N = 2048 ring -------------------------------------------------------------------------------------------------------------
class Ring2:
    def __init__(self, engine):
        rng = np.random.default_rng(2800)
        self.E = {s: es.edge_words(11, s) for s in SHIFTS}
        self.b_rows = {s: es.sweep_rows(self.E[s], "b", n, rng) for s in SHIFTS}
        self.a_rows = {s: bbar_identity(es.sweep_rows(self.E[s], "a", n, rng), 11, s) for s in (0, 2)}
        self.tv = {s: rng.integers(0, 1 << 64, N2, dtype=np.uint64) for s in SHIFTS}
        self.off = {s: int(rng.integers(1, 1 << 32)) for s in SHIFTS}
        self.op = {s: engine.api.lvl2_define_gate((1, 0, 0), self.off[s], self.tv[s], nout=1 << s) for s in SHIFTS}


@pytest.fixture(scope="module")
def ring2(engine2, tidy):
    return Ring2(engine2)


def ring_rotate(engine, op, x, steps):
    count = x.shape[0]
    dacc = engine.api.DeviceBuffer(count * 2 * N2 * 2)
    if op is None:
        engine.api.lvl2_blind_rotate_batch(_upload(engine, x), dacc, count, steps)
    else:
        engine.api.lvl2_user_rotate_batch(op, _upload(engine, x), dacc, count, steps=steps)
    engine.Synchronize()
    return dacc.download().view(np.uint64).reshape(count, 2 * N2)


def test_ring_bbar_of_the_built_in_rotation(engine2, ring2, br2_kernel):
    """lvl2_blind_rotate_batch, 0 steps: (0, X^bbar 2^61) at both edge words of all 4096 values of bbar"""
    rows, E = ring2.b_rows[0], ring2.E[0]
    want = once("mu2", lambda: np.stack([es.start_acc("const", b, 0, 11, bits=64, const=ol.MU2) for b in rows[:, n]]))
    same(ring_rotate(engine2, None, rows, 0), want, E, "b", "built-in 2^61, " + br2_kernel)


@pytest.mark.parametrize("s", SHIFTS)
def test_ring_bbar_of_user_gates(engine2, ring2, br2_kernel, s):
    """lvl2_user_rotate_batch, 0 steps: (0, X^bbar TV) of a random 64-bit row, single-output and with 2, 4, 8 outputs"""
    rows, E = ring2.b_rows[s], ring2.E[s]
    want = once(("tv2", s), lambda: np.stack([es.start_acc("tv", b, s, 11, bits=64, tv=ring2.tv[s]) for b in rows[:, n]]))
    same(ring_rotate(engine2, ring2.op[s], with_offset(rows, ring2.off[s]), 0), want, E, "b", "ring user gate, s = %d, %s" % (s, br2_kernel))


def test_ring_abar_of_the_built_in_first_step(engine2, keys2, ring2, br2_kernel):
    """lvl2_blind_rotate_batch, 1 step from the constant 2^61 against orc2_blind_rotate: both edge words of all 4096 values of abar"""
    rows, E = ring2.a_rows[0], ring2.E[0]
    want = once("mu2 step", lambda: np.stack(l2.on_threads(lambda g: keys2.blind_rotate(rows[g], 1), rows.shape[0])))
    same(ring_rotate(engine2, None, rows, 1), want, E, "a", "built-in 2^61, one step, " + br2_kernel)


# one reference step of the ring costs about 2 ms of CPU, so the two edges of the 4096 exponents are two cases of 4096 rows
RING_STEP_CASES = {"low": (0, slice(0, None, 2)), "high": (0, slice(1, None, 2)), "s2": (2, slice(None))}


@pytest.mark.parametrize("case", list(RING_STEP_CASES))
def test_ring_abar_of_the_first_step(engine2, keys2, ring2, br2_kernel, case):
    """lvl2_user_rotate_batch, 1 step from a random row left in place: every abar at its low edge word, at its high edge word, and the
    coarse grid of a four-output definition at both"""
    s, pick = RING_STEP_CASES[case]
    rows, E, tv = ring2.a_rows[s][pick], ring2.E[s], ring2.tv[s]
    step = (lambda g: l2.blind_rotate_tv(keys2, rows[g], tv, 1)) if s == 0 else (lambda g: m2.blind_rotate_tv_multi(keys2, rows[g], tv, s, 1))
    want = once(("step2", case), lambda: np.stack(l2.on_threads(step, rows.shape[0])))
    got = ring_rotate(engine2, ring2.op[s], with_offset(rows, ring2.off[s]), 1)
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        g = int(bad[0])
        w = int(np.flatnonzero(got[g] != want[g])[0])
        pytest.fail("ring, one step, %s, %s: %d of %d rows differ; first: row %d, a word %#x (abar %d), word %d" % (
            case, br2_kernel, bad.size, rows.shape[0], g, int(rows[g, 0]), es.ms_abar(rows[g, 0], 11, s), w))


# ---- the parameter sets ------------------------------------------------------------------------------------------------------------
class SetSweep:
    def __init__(self, engine, name):
        api = engine.api
        self.name, self.C, self.idx = name, pc.Checker(name, seed=5), api.ps_index(name)
        C = self.C
        api.ps_initialize(self.idx, C.K.bk, C.K.ksk)
        rng = np.random.default_rng(2900 + self.idx)
        self.E = {s: es.edge_words(C.nbit, s) for s in SHIFTS}
        self.b_rows = {s: es.sweep_rows(self.E[s], "b", C.n, rng) for s in SHIFTS}
        self.a_rows = {s: bbar_identity(es.sweep_rows(self.E[s], "a", C.n, rng), C.nbit, s) for s in (0, 2)}
        self.tv = {s: words32(rng, C.N) for s in SHIFTS}
        self.off = {s: int(rng.integers(1, 1 << 32)) for s in SHIFTS}
        self.op = {s: api.ps_define_gate(self.idx, (1, 0, 0), self.off[s], self.tv[s], nout=1 << s) for s in SHIFTS}
        self.ref = {}

    def once(self, key, make):
        if key not in self.ref:
            self.ref[key] = make()
        return self.ref[key]

    def rotate(self, engine, s, x, steps):
        C, count = self.C, x.shape[0]
        dacc = up(engine, np.full(count * C.acc_words, FILL, np.uint32))
        if s is None:
            engine.api.ps_blind_rotate_batch(self.idx, up(engine, x), dacc, count, steps)
        else:
            engine.api.ps_user_rotate(self.idx, self.op[s], up(engine, x), dacc, count, steps=steps)
        engine.Synchronize()
        return dacc.download().reshape(count, C.acc_words)


@pytest.fixture(scope="module", params=ol.SETS)
def pset(request, engine, tidy):
    return SetSweep(engine, request.param)


@pytest.fixture(params=["wg", "batch"])
def ps_kernel(request, engine):
    engine.api.set_option("ps_batch_threshold", 1 << 30 if request.param == "wg" else 1)
    yield request.param
    engine.api.set_option("ps_batch_threshold", -1)


def test_sets_bbar(engine, pset, ps_kernel):
    """0 steps on both kernels of every set: <TV = false> through ps_blind_rotate_batch, <TV = true> through ps_user_rotate with a
    random row under s = 0 .. 3; the k mask polynomials stay zero"""
    C = pset.C
    rows, E = pset.b_rows[0], pset.E[0]
    want = pset.once("mu", lambda: np.stack([es.start_acc("mu", b, 0, C.nbit, k=C.k) for b in rows[:, C.n]]))
    same(pset.rotate(engine, None, rows, 0), want, E, "b", "%s %s: built-in mu" % (pset.name, ps_kernel))
    for s in SHIFTS:
        rows, E = pset.b_rows[s], pset.E[s]
        want = pset.once(("tv", s), lambda: np.stack([es.start_acc("tv", b, s, C.nbit, k=C.k, tv=pset.tv[s]) for b in rows[:, C.n]]))
        got = pset.rotate(engine, s, with_offset(rows, pset.off[s]), 0)
        same(got, want, E, "b", "%s %s: user gate, s = %d" % (pset.name, ps_kernel, s))
        assert not got[:, :C.k * C.N].any(), "%s %s: a mask polynomial of the first accumulator is not zero" % (pset.name, ps_kernel)


def set_step_reference(pset, s):
    C, rows, tv = pset.C, pset.a_rows[s], pset.tv[s]
    bk0 = np.ascontiguousarray(C.bk_cmux[:C.step_words])

    def one(g):
        acc = es.start_acc("tv", rows[g, C.n], s, C.nbit, k=C.k, tv=tv)
        rot = es.rotate_many(acc.reshape(C.k + 1, C.N), es.ms_abar(rows[g, 0], C.nbit, s), C.N).reshape(-1)
        res = np.empty(C.acc_words, np.uint32)
        C.L.orc_cmux(res, bk0, rot, acc)
        return res
    return np.stack(pc.on_threads(one, rows.shape[0]))


def test_sets_abar_of_the_first_step(engine, pset, ps_kernel):
    """ps_user_rotate, 1 step from a random row left in place: both edge words of every abar, and the coarse grid of s = 2; and
    ps_blind_rotate_batch, 1 step from the constant mu, against the set's orc_blind_rotate"""
    C, rows = pset.C, pset.a_rows[0]
    want = pset.once("mu step", lambda: np.stack(pc.on_threads(lambda g: C.K.blind_rotate(rows[g], 1), rows.shape[0])))
    same(pset.rotate(engine, None, rows, 1), want, pset.E[0], "a", "%s %s: built-in mu, one step" % (pset.name, ps_kernel))
    for s in (0, 2):
        rows, E = pset.a_rows[s], pset.E[s]
        want = pset.once(("step", s), lambda: set_step_reference(pset, s))
        same(pset.rotate(engine, s, with_offset(rows, pset.off[s]), 1), want, E, "a", "%s %s: one step, s = %d" % (pset.name, ps_kernel, s))
