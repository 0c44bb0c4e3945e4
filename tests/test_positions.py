"""tests/positions.py on the CPU: the helper that tests/test_gpu_positions.py relies on sees the faults it is there for (one wrong
word, swapped neighbours, a row nobody wrote, a row that holds another input's result), the periods it tiles with reach every
slot of every grouping, and it runs for real on the optimised CPU gate path against the oracle."""
import numpy as np
import pytest

import oracle_lib as ol
import positions as pos


def _case(D=67, count=300, words=631, seed=1):
    rng = np.random.default_rng(seed)
    want = rng.integers(0, 2**32, size=(D, words), dtype=np.uint64).astype(np.uint32)
    return want, pos.tile(want, count)


def test_tile_is_row_g_carries_input_g_mod_d():
    want, got = _case(D=7, count=30, words=5)
    for g in range(30):
        assert np.array_equal(got[g], want[g % 7])
    assert all(not np.array_equal(got[g], got[g + 1]) for g in range(29))


@pytest.mark.parametrize("bad", [1, 4, 5, 8, 13, 16, 26, 40, 64, 104, 256])
def test_tile_refuses_a_period_that_divides_a_grouping_or_is_no_prime(bad):
    with pytest.raises(AssertionError):
        pos.tile(np.zeros((bad, 3), np.uint32), 100)


def test_accepts_the_exact_array():
    want, got = _case()
    pos.assert_every_row(got, want, "exact", groupings=(8, 16))
    assert pos.report(got, want, "exact") is None


def test_one_flipped_bit_in_one_row():
    want, got = _case()
    got[214, 630] ^= 1 << 17
    with pytest.raises(AssertionError) as e:
        pos.assert_every_row(got, want, "flip", groupings=(8, 16, 512))
    msg = str(e.value)
    assert "1 of 300 rows" in msg and "first rows: [214]" in msg
    assert "rows mod 8: [6]" in msg and "rows mod 16: [6]" in msg and "rows mod 512: [214]" in msg
    assert "row 214, first wrong word 630" in msg
    assert "row 214 (input 13): arithmetic" in msg and "(1 of 631 words wrong)" in msg


def test_two_neighbouring_rows_swapped():
    want, got = _case()
    got[[101, 102]] = got[[102, 101]]
    with pytest.raises(AssertionError) as e:
        pos.assert_every_row(got, want, "swap", groupings=(8,))
    msg = str(e.value)
    assert "2 of 300 rows" in msg and "first rows: [101, 102]" in msg and "rows mod 8: [5, 6]" in msg
    assert "row 101 (input 34): routing: the words expected for distinct input 35" in msg
    assert "row 102 (input 35): routing: the words expected for distinct input 34" in msg


def test_one_row_left_at_the_poison_value():
    want, got = _case()
    got[299] = pos.POISON
    with pytest.raises(AssertionError) as e:
        pos.assert_every_row(got, want, "unwritten", groupings=(16,))
    msg = str(e.value)
    assert "1 of 300 rows" in msg and "first rows: [299]" in msg and "rows mod 16: [11]" in msg
    assert "row 299 (input 31): never written" in msg


def test_one_row_equal_to_another_inputs_expectation():
    want, got = _case()
    got[7] = want[50]
    with pytest.raises(AssertionError) as e:
        pos.assert_every_row(got, want, "routed")
    msg = str(e.value)
    assert "first rows: [7]" in msg and "row 7 (input 7): routing: the words expected for distinct input 50" in msg
    assert "rows [50]" in msg          # where that input sits near the wrong row


def test_uint64_rows_and_trailing_dimensions():
    rng = np.random.default_rng(3)
    want = rng.integers(0, 2**63, size=(7, 3, 5), dtype=np.uint64)
    got = pos.tile(want, 23)
    pos.assert_every_row(got, want, "u64")
    got[22, 2, 4] += np.uint64(1)
    msg = pos.report(got, want, "u64", groupings=(4,))
    assert "first rows: [22]" in msg and "rows mod 4: [2]" in msg and "first wrong word 14" in msg
    got = pos.tile(want, 23)
    got[3] = pos.poison((3, 5), np.uint64)
    assert "row 3 (input 3): never written" in pos.report(got, want, "u64")
    assert pos.report(got.astype(np.uint32), want, "u64") is not None      # another word size is a mismatch, not a cast


def test_a_missing_or_extra_row_cannot_pass():
    want, got = _case(count=68)
    assert pos.report(got[:67], want, "short") is None          # 67 rows ARE right: the caller passes all rows of the launch ...
    shifted = np.concatenate([got[1:], got[:1]])
    assert "67 of 68 rows" in pos.report(shifted, want, "shifted")     # ... and a shift of them is wrong on every row but the one that wraps


@pytest.mark.parametrize("path", sorted(pos.PATHS))
def test_the_period_drifts_through_every_slot_of_every_grouping(path):
    """What "the period drifts through every slot" rests on: within the largest count of a path the rows cover every slot of every
    grouping no larger than that count, and every distinct input meets every slot of the groupings inside a workgroup (8, 12, 16
    rotations or ciphertexts, 64) -- so a fault bound to one slot meets every kind of input, the corner inputs included."""
    D, largest = pos.PATHS[path]
    assert D in pos.PRIMES
    pos.check_period(D)
    for m in pos.GROUPINGS + (2 * 256, 8 * 40, 8 * 104):
        if m <= largest:
            assert pos.every_slot_is_visited(D, largest, m), (path, D, m)
    for m in (4, 8, 12, 16, 64):
        if D * m <= largest:
            assert pos.every_input_visits_every_slot(D, largest, m), (path, D, m)
    assert pos.every_input_visits_every_slot(D, largest, 4) and pos.every_input_visits_every_slot(D, largest, 8)
    # neighbouring rows differ, and so do rows one workgroup apart
    for step in (1, 4, 8, 12, 16, 64, 256, 2048):
        assert step % D


def test_option_guard_restores_defaults_even_after_a_failure():
    class Api:
        def __init__(self):
            self.calls = []

        def set_option(self, k, v):
            self.calls.append((k, v))

    api = Api()
    with pytest.raises(RuntimeError):
        with pos.options(api, dict(ll_threshold=0, cus_override=40, lvl0_ring=2048, tail_split=0)):
            raise RuntimeError("inside")
    assert api.calls == [("ll_threshold", 0), ("cus_override", 40), ("lvl0_ring", 2048), ("tail_split", 0),
                         ("ll_threshold", -1), ("cus_override", 0), ("lvl0_ring", 1024), ("tail_split", 1)]
    with pytest.raises(AssertionError):
        with pos.options(api, dict(no_such_option=1)):
            pass


def test_helper_on_the_cpu_fast_path_against_the_oracle(oracle, keys):
    """The helper run for real: fast_gate_batch (oracle/cpu_fast.c, blocks of gates through shared key rows) against
    orc_gate_batch on a tiled batch of 300 mixed two-input gates, every row; then one row of the fast path's output damaged."""
    D, count = 17, 300
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, size=(2, D)).astype(np.uint8)
    ins = [keys.encrypt(bits[i], 0, seed=6100 + i) for i in range(2)]
    ops = (np.arange(D) % 10).astype(np.int32)                 # the ten two-input ops (the fast path has no MUX / NOT / COPY)
    want = keys.gate_batch(ops, 0, ins[0], ins[1])
    t_ops, t0, t1 = pos.tile(ops, count), pos.tile(ins[0], count), pos.tile(ins[1], count)
    ek = oracle.fast_evalkey_create(keys.bk, keys.ksk)
    try:
        got = pos.poison((count, ol.n + 1))
        assert oracle.fast_gate_batch(ek, t_ops, 1, count, got.ravel(), t0.ravel(), t1.ravel(), 0) == 0
    finally:
        oracle.fast_evalkey_destroy(ek)
    pos.assert_every_row(got, want, "fast_gate_batch, 300 mixed gates", groupings=(8, 16))
    got[123, 0] += np.uint32(1)
    assert "first rows: [123]" in pos.report(got, want, "damaged")
