"""CPU checks of tests/stream_contract.py: the counts of tests/test_gpu_stream_contract.py do make every grow-only pool regrow in the
middle of a chain and reuse it shrunk afterwards, the library's constants are the ones the arithmetic uses, and the values a host array
is overwritten with are valid and different."""
import re

import numpy as np
import pytest

import footprint as fp
import stream_contract as sc


def test_constants_are_the_librarys():
    assert fp.csrc_constant("kKsMmRows", ("kernels_ks2.hip.h",)) == sc.KS_MM_ROWS
    text = open(fp.CSRC + "/capi.hip").read()
    # open_scratch's slack: a quarter plus 1 MiB
    assert re.search(r"const size_t want = bytes \+ bytes / 4 \+ \(1 << 20\);", text)
    ks2 = open(fp.CSRC + "/kernels_ks2.hip.h").read()
    assert "constexpr int kKsMmSteps = KsShapeDefault::kn / 2;" in ks2
    assert "return (count + kKsMmRows - 1) / kKsMmRows * kKsMmSteps * 64 * sizeof(uint32_t);" in ks2
    assert sc.KS_MM_TILE_BYTES == sc.N // 2 * 64 * 4
    common = open(fp.CSRC + "/kernels_common.hip.h").read()
    body = re.search(r"struct LinDesc \{(.*?)\n\};", common, re.S).group(1)
    assert len(re.findall(r"uint32_t\*", body)) == 3 and sc.LIN_DESC == 3 * 8 + 4 * 4


@pytest.mark.parametrize("counts", [sc.GATE_COUNTS, sc.SHORT_COUNTS])
def test_gate_counts_regrow_the_workspace_twice_and_reuse_it_twice(counts):
    assert sc.grows([sc.gate_need(c) for c in counts]) == [True, True, False, True, False]
    # a MUX costs two rotations: the regrowths stay where they are
    assert sc.grows([sc.gate_need(c, 2) for c in counts]) == [True, True, False, True, False]


def test_fourfold_step_regrows_from_56_gates_on():
    first = next(c for c in range(1, 1000) if sc.grows([sc.gate_need(c), sc.gate_need(4 * c)])[1])
    assert first == 56
    assert all(sc.grows([sc.gate_need(c), sc.gate_need(4 * c)])[1] for c in (56, 256, 1024, 4096))


def test_keyswitch_counts_regrow_the_digit_words():
    r = sc.KS_MM_ROWS
    assert sc.KS_COUNTS == (1, r + 1, 1, 4 * r + 4)
    assert sc.grows([sc.ks_digit_bytes(c) for c in sc.KS_COUNTS], slack=False) == [True, True, False, True]
    assert [sc.ks_digit_bytes(c) // sc.KS_MM_TILE_BYTES for c in sc.KS_COUNTS] == [1, 2, 1, 5]
    # behind the gates of the chain the digit words regrow with the workspace
    assert sc.grows([sc.ks_digit_bytes(c) for c in sc.GATE_COUNTS], slack=False) == [True, True, False, True, False]


def test_round_robin():
    assert sc.round_robin([3, 2]) == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2)]
    assert sc.round_robin([]) == [] and sc.round_robin([1, 1, 1, 1]) == [(k, 0) for k in range(4)]


def test_other_values_are_valid_and_different():
    ops = np.arange(14, dtype=np.int32)
    alt = sc.other_ops(ops)
    arity = lambda op: 1 if op >= 12 else 3 if op >= 10 else 2  # noqa: E731
    assert all(arity(a) == arity(o) and a != o for a, o in zip(alt, ops))
    e = np.array([0, 1, 2047, 1024], np.int32)
    alt = sc.other_in_range(e, 2048, 1031)
    assert ((alt >= 0) & (alt < 2048) & (alt != e)).all()
    with pytest.raises(AssertionError):
        sc.other_in_range(np.array([2048]), 2048, 1)


def test_differs_in_every_row():
    a = np.arange(12).reshape(3, 4)
    b = a.copy()
    b[:, 0] += 1
    assert sc.differs_in_every_row(a, b)
    b[1] = a[1]
    assert not sc.differs_in_every_row(a, b)
    assert not sc.differs_in_every_row(a, a[:2])
