"""The tail of a CMux step of blind_rotate_kernel -- the last inverse pass with the four-operation root products, the reductions
placed register by register and the lift in FP64 operations only (ntt_r4.h: InverseRootTail, ntt_wave.h: lift_add_fp64): accumulator
words after 1, 2, 3 and all n steps against the oracle, word for word.

One rotation, and nine: on the shape with 8 rotations per workgroup nine are one full workgroup -- both the early and the late
half of its waves -- and a second one with a single rotation beside seven waves that only serve the row pipeline; on the shape
with 4, three workgroups.  Both instantiations: without a table (the built-in gates) and from a table array (<true>).  Rotation 0
has abar = 0 in its first three steps, rotation 1 in its second, rotation 2 in every seventh: steps that add nothing.

The extreme case drives the sums to the bound the exactness of the FP64 field rests on, (k+1) l N (Bg/2) 2^31: every key word is
0x80000000 and step 0 sees a constant polynomial whose digits are all -32 (table A = B = c with -2 c = -offset, bbar = 0,
abar = N, so that X^abar acc - acc = -2 c in every coefficient).  The lift then sees the largest values it ever can."""
import types

import numpy as np
import pytest

import lut_checker as lc
import oracle_lib as ol
from test_gpu_user_gates import run_batch, set_shape, up

pytestmark = pytest.mark.gpu

N, n = ol.N, ol.n
NBIT = N.bit_length() - 1
COUNT = 9
STEPS = [1, 2, 3, n]
FILL = 0xA5A5A5A5
BGBIT, L = 6, 3
OFFSET = sum(1 << (32 - i * BGBIT + BGBIT - 1) for i in range(1, L + 1)) + (1 << (32 - L * BGBIT - 1))
SIGNMASK = sum(1 << (32 - i * BGBIT + BGBIT - 1) for i in range(1, L + 1))


class Data:
    """the inputs, and the references of (kind, steps): computed once for nine rotations, the first of which is the case of one"""

    def __init__(self, keys, oracle):
        rng = np.random.default_rng(4100)
        self.keys, self.oracle = keys, oracle
        self.x = rng.integers(0, 1 << 32, size=(COUNT, n + 1), dtype=np.uint64).astype(np.uint32)
        self.x[0, 0:3] = 0
        self.x[1, 1] = 0
        self.x[2, 0:n:7] = 0
        self.tables = rng.integers(0, 1 << 32, size=(COUNT, 2 * N), dtype=np.uint64).astype(np.uint32)
        self._want = {}

    def plain(self, g, steps):
        want = np.zeros(2 * N, np.uint32)
        self.oracle.orc_blind_rotate(self.keys.ek, want, np.ascontiguousarray(self.x[g]), steps)
        return want

    def want(self, kind, steps):
        if (kind, steps) not in self._want:
            fn = self.plain if kind == "plain" else (lambda g, s: lc.lut_rotate(self.keys, self.x[g], self.tables[g], 0, s))
            self._want[(kind, steps)] = np.stack(lc.on_threads(lambda g: fn(g, steps), COUNT))
        return self._want[(kind, steps)]


@pytest.fixture(scope="module")
def data(keys, oracle):
    return Data(keys, oracle)


def rotate(engine, kind, x, tables, count, steps):
    dacc = up(engine, np.full(count * 2 * N, FILL, np.uint32))
    if kind == "plain":
        engine.blind_rotate_batch(up(engine, x[:count]), dacc, count, steps)
    else:
        engine.api.lut_rotate_batch(up(engine, x[:count]), up(engine, tables[:count]), dacc, count, count, src=None, nout=1, steps=steps)
    engine.Synchronize()
    return dacc.download().reshape(count, 2 * N)


def test_zero_steps_are_zero(data):
    """abar of the steps named above is 0 as the kernel's modulus switch computes it, and of their neighbours it is not"""
    abar = ((data.x[:, :n].astype(np.uint64) + (1 << (32 - 2 - NBIT))) >> (32 - 1 - NBIT)) & (2 * N - 1)
    assert not abar[0, 0:3].any() and abar[0, 3] and not abar[1, 1] and abar[1, 0] and abar[1, 2] and not abar[2, 0:n:7].any()
    assert abar[3:, :3].all()


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("kind", ["plain", "table"])
@pytest.mark.parametrize("count", [1, COUNT])
@pytest.mark.parametrize("shape", ["batch", "half"])
def test_accumulator_words(engine, data, shape, count, kind, steps):
    want = data.want(kind, steps)[:count]
    set_shape(engine.api, shape)
    try:
        got = rotate(engine, kind, data.x, data.tables, count, steps)
    finally:
        set_shape(engine.api, None)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s, %d rotations, %s, %d steps: %d words differ, first at (rotation, word) %s" % (
        shape, count, kind, steps, len(bad), tuple(bad[0]))


@pytest.mark.parametrize("count", [1, COUNT])
def test_nand_gate(engine, keys, count):
    """the whole built-in gate: 630 steps, sample extraction and key switch"""
    bits = np.random.default_rng(4101).integers(0, 2, size=(2, count)).astype(np.uint8)
    a, b = keys.encrypt(bits[0], 0, seed=4102), keys.encrypt(bits[1], 0, seed=4103)
    got = run_batch(engine, engine.api.NAND, 0, [a, b], count)
    assert np.array_equal(got, keys.gate_batch(engine.api.NAND, 0, a, b))
    assert list(keys.decrypt(got, 0)) == list(1 - bits[0] * bits[1])


def extreme_inputs():
    c = (OFFSET // 2) & 0xFFFFFFFF
    x = np.random.default_rng(4104).integers(0, 1 << 32, size=(COUNT, n + 1), dtype=np.uint64).astype(np.uint32)
    x[:, 0] = N << (32 - 1 - NBIT)          # abar = N at step 0
    x[:, n] = 0                             # bbar = 0: the accumulator starts as the table itself
    tables = np.full((COUNT, 2 * N), c, np.uint32)
    return x, tables


def test_extreme_inputs_have_every_digit_at_minus_32():
    x, tables = extreme_inputs()
    acc = tables[0, :N].astype(np.int64)
    temp = ((-acc - acc + OFFSET) & 0xFFFFFFFF) ^ SIGNMASK           # X^N acc = -acc
    for d in range(L):
        field = (temp >> (32 - (d + 1) * BGBIT)) & ((1 << BGBIT) - 1)
        assert np.all(field - ((field >> (BGBIT - 1)) << BGBIT) == -(1 << (BGBIT - 1)))
    assert OFFSET % 2 == 0 and lc.mc.ms_abar(x[0, 0], 0) == N and lc.mc.ms_bbar(x[0, n], 0) % (2 * N) == 0


def test_extreme_sums(engine, keys, oracle):
    """every key word 0x80000000, every digit of step 0 equal to -32: the sums reach (k+1) l N (Bg/2) 2^31.  One and three steps on
    both launch shapes, under one exchange of the key."""
    x, tables = extreme_inputs()
    bk = np.full(keys.bk.size, 0x80000000, np.uint32)
    extreme = types.SimpleNamespace(L=oracle, bk=bk)
    want = {steps: np.stack([lc.lut_rotate(extreme, x[g], tables[g], 0, steps) for g in range(COUNT)]) for steps in (1, 3)}
    got = {}
    engine.CleanUp()
    engine.SetGPUNum(1)
    engine.Initialize(bk, keys.ksk)
    try:
        for shape in ("batch", "half"):
            set_shape(engine.api, shape)
            for steps in (1, 3):
                got[(shape, steps)] = rotate(engine, "table", x, tables, COUNT, steps)
    finally:
        set_shape(engine.api, None)
        engine.CleanUp()
        engine.SetGPUNum(1)
        engine.Initialize(keys.bk, keys.ksk)
    for (shape, steps), words in got.items():
        bad = np.argwhere(words != want[steps])
        assert not len(bad), "%s, %d steps: %d words differ, first at (rotation, word) %s" % (shape, steps, len(bad), tuple(bad[0]))
