"""The first TRGSW row of a CMux step of blind_rotate_kernel WRITES the two NTT-domain sums instead of adding to zeroed ones, and the
row pipeline keeps its source address in scalar registers: accumulator words after 1, 2 and all n steps against the oracle, word for
word, at the places where that could show.

Nine rotations: on the shape with 8 rotations per workgroup that is two workgroups, the second with seven waves that only serve the
row pipeline (on the shape with 4, three workgroups, the last with one rotation).  Step 0 of rotations 0 .. 4 has
abar = 0, 1, N - 1, N and 2N - 1.  Without a table the accumulator starts as (0, X^bbar TV): component 0 is all zero at step 0 in
EVERY rotation, so every digit of the first row is zero and the sum it writes must be exactly 0 (the plain-gate case).  With a table
array (the <true> instantiation) it starts as X^bbar (A, B); table 5 has A = 0 and is that case there, the others have random A."""
import numpy as np
import pytest

import lut_checker as lc
import oracle_lib as ol
from test_gpu_user_gates import set_shape, up

pytestmark = pytest.mark.gpu

N, n = ol.N, ol.n
NBIT = N.bit_length() - 1
COUNT = 9
STEPS = [1, 2, n]
ABAR0 = [0, 1, N - 1, N, 2 * N - 1]
ZERO_A = 5
FILL = 0xA5A5A5A5


class Data:
    """the inputs, and the references of (kind, steps): computed once, shared by both launch shapes"""

    def __init__(self, keys, oracle):
        rng = np.random.default_rng(3900)
        self.keys, self.oracle = keys, oracle
        self.x = rng.integers(0, 1 << 32, size=(COUNT, n + 1), dtype=np.uint64).astype(np.uint32)
        for g, abar in enumerate(ABAR0):
            self.x[g, 0] = abar << (32 - 1 - NBIT)          # the modulus switch rounds it to exactly abar
        self.tables = rng.integers(0, 1 << 32, size=(COUNT, 2 * N), dtype=np.uint64).astype(np.uint32)
        self.tables[ZERO_A, :N] = 0
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


def test_step_zero_inputs(data):
    """the inputs are what the cases above say: abar of step 0 as the kernel's modulus switch computes it, the zero component"""
    abar = ((data.x[:, 0].astype(np.uint64) + (1 << (32 - 2 - NBIT))) >> (32 - 1 - NBIT)) & (2 * N - 1)
    assert list(abar[:len(ABAR0)]) == ABAR0
    assert not data.tables[ZERO_A, :N].any() and data.tables[ZERO_A, N:].any()
    assert all(data.tables[g, :N].any() for g in range(COUNT) if g != ZERO_A)


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("kind", ["plain", "table"])
@pytest.mark.parametrize("shape", ["batch", "half"])
def test_accumulator_words(engine, data, shape, kind, steps):
    api = engine.api
    want = data.want(kind, steps)
    dx = up(engine, data.x)
    dacc = up(engine, np.full(COUNT * 2 * N, FILL, np.uint32))
    set_shape(api, shape)
    try:
        if kind == "plain":
            engine.blind_rotate_batch(dx, dacc, COUNT, steps)
        else:
            api.lut_rotate_batch(dx, up(engine, data.tables), dacc, COUNT, COUNT, src=None, nout=1, steps=steps)
        engine.Synchronize()
    finally:
        set_shape(api, None)
    got = dacc.download().reshape(COUNT, 2 * N)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s, %s, %d steps: %d words differ, first at (rotation, word) %s" % (shape, kind, steps, len(bad), tuple(bad[0]))
