"""CPU tests of tests/argument_sweeps.py: the references of tests/test_gpu_argument_sweeps.py are pinned to the checkers the suite
already trusts before any GPU word is compared with them.  spread_all (incremental, all 7262 pairs) equals lut_checker.spread (one
term at a time) wherever that is affordable and at every edge of the pair domain; the delta input's Spread is the window mask
itself; pack_checker.rotate is multiplication by X^e; the packing target lists name every position."""
import numpy as np

import argument_sweeps as sw
import lut_checker as lc
import pack_checker as pk

N = sw.N


def test_pair_count_and_bands():
    pairs = sw.spread_pairs()
    assert len(pairs) == sw.SPREAD_PAIRS == 7262 == sum(N // s for s in range(1, N + 1))
    assert len(set(pairs)) == len(pairs) and all(s >= 1 and r >= 1 and s * r <= N for s, r in pairs)
    assert set(pairs) == {(s, r) for s in range(1, N + 1) for r in range(1, N + 1) if s * r <= N}
    # the bands are consecutive, cover every stride and hold at most 32 MB of output each (3 TRLWEs of 8 KiB per pair)
    assert sw.SPREAD_BANDS[0][0] == 1 and sw.SPREAD_BANDS[-1][1] == N
    assert all(sw.SPREAD_BANDS[i][1] + 1 == sw.SPREAD_BANDS[i + 1][0] for i in range(len(sw.SPREAD_BANDS) - 1))
    sizes = [len(sw.spread_pairs(range(lo, hi + 1))) for lo, hi in sw.SPREAD_BANDS]
    assert sum(sizes) == 7262 and max(sizes) * 3 * 2 * N * 4 <= 32 << 20, sizes
    assert set(sw.EXISTING_SPREADS) <= set(pairs)
    # what the eight pairs of the suite left out is in the domain: big > 1, len = 1, an odd stride short of N
    assert any(N % s > 1 for s, _ in pairs) and any(s > N // 2 for s, _ in pairs) and any(s % 2 and s * r < N - s for s, r in pairs)


def test_recorded_pairs_and_their_order():
    rec = sw.recorded_spread_pairs()
    assert len(rec) == 66 == len(set(rec)) and set(rec) <= set(sw.spread_pairs())
    order = sw.recorded_spread_order(2500)
    assert sorted(order) == sorted(rec) and order == sw.recorded_spread_order(2500)
    for a, b in zip(order, order[1:]):
        assert a[0] != b[0] and a[1] != b[1], (a, b)
    assert order != sw.recorded_spread_order(2501)


def test_spread_all_equals_the_checker():
    """the 8 pairs the suite had, every pair with reps <= 3, every stride > N / 2, every pair with stride reps in {N - 1, N}, and 64
    random pairs, on the three TRLWEs the GPU sweep uses: every word"""
    x = sw.sweep_inputs(2400)
    pairs = sw.spread_pairs()
    rng = np.random.default_rng(2401)
    chosen = set(sw.EXISTING_SPREADS)
    chosen |= {p for p in pairs if p[1] <= 3 or p[0] > N // 2 or p[0] * p[1] in (N - 1, N)}
    chosen |= {pairs[i] for i in rng.choice(len(pairs), size=64, replace=False)}
    assert len([p for p in pairs if p[0] > N // 2]) == N // 2 and len(chosen) >= 1877 + 64
    seen = 0
    for (stride, reps), w in sw.spread_all(x.reshape(6, N)):
        if (stride, reps) not in chosen:
            continue
        seen += 1
        for g in range(3):
            want = lc.spread(x[g], stride, reps)
            assert np.array_equal(w[2 * g:2 * g + 2].reshape(2 * N), want), (stride, reps, g)
    assert seen == len(chosen)


def test_spread_all_order_and_restriction():
    x = sw.sweep_inputs(2400)[:1].reshape(2, N)
    assert [p for p, _ in sw.spread_all(x)] == sw.spread_pairs()
    some = [1, 3, 341, 700, 1024]
    part = dict(sw.spread_all(x, some))
    assert list(part) == sw.spread_pairs(some)
    full = {p: w for p, w in sw.spread_all(x) if p[0] in some}
    assert all(np.array_equal(part[p], full[p]) for p in part)


def test_delta_input_is_the_window_mask():
    """for all pairs: Spread of the delta TRLWE is exactly `reps` coefficients of magnitude 1 at spacing `stride`, with the sign the
    negacyclic wrap gives each"""
    x = sw.sweep_inputs(2400)
    assert np.count_nonzero(x[2]) == 2 and x[2, 0] == 1 and x[2, 2 * N - 1] == sw.M32
    count = 0
    for (stride, reps), w in sw.spread_all(x[2].reshape(2, N)):
        count += 1
        for j, (at, word) in enumerate(((0, 1), (N - 1, sw.M32))):
            nz = np.flatnonzero(w[j])
            assert len(nz) == reps and np.all((w[j, nz] == 1) | (w[j, nz] == sw.M32)), (stride, reps, j)
            heads = nz[~np.isin((nz - stride) % N, nz)]                           # a chain of steps of `stride` around the ring ...
            head = int(heads[0]) if len(heads) else int(nz[0])                    # ... closed when stride reps = N
            assert len(heads) <= 1 and np.array_equal(np.sort((head + np.arange(reps) * stride) % N), nz), (stride, reps, j)
            assert np.array_equal(w[j], sw.delta_window(stride, reps, at, word)), (stride, reps, j)
    assert count == 7262


def test_describe_spread_failure_names_the_branch():
    assert "t >= reps" in sw.describe_spread_failure(1, 1, 0, 5) and "big = 0" in sw.describe_spread_failure(1, 1, 0, 5)
    msg = sw.describe_spread_failure(3, 341, 5, 1000)
    assert "big = 1" in msg and "len = 341" in msg and "negated" in msg and "TRLWE 2" in msg
    msg = sw.describe_spread_failure(700, 1, 1, 0)
    assert "len = 1" in msg and "big = 324" in msg and "t < reps" in msg and "jmax" in msg


def test_pack_rotate_is_multiplication_by_a_monomial():
    """pack_checker.rotate(row, e) for ALL e in [0, N) equals schoolbook multiplication by X^e"""
    row = np.random.default_rng(2402).integers(0, 1 << 32, size=2 * N, dtype=np.uint64).astype(np.uint32)
    row[[0, 1, N - 1, N, 2 * N - 1]] = (0x80000000, 0xFFFFFFFF, 1, 0, 0x80000000)
    for e in range(N):
        assert np.array_equal(pk.rotate(row, e), sw.schoolbook_rotate(row, e)), e


def test_pack_targets_name_every_position():
    t = sw.pack_targets(2403)
    dst, pos, count_out = t["isolated"]
    assert count_out == N + 1 == len(dst) and np.array_equal(dst, np.arange(N + 1))
    assert sorted(pos[:N].tolist()) == list(range(N)) and pos[N] == 0
    dst, pos, count_out = t["shared"]
    assert count_out == 2 and len(dst) == N + 1 and np.count_nonzero(dst == 1) == 1 and np.count_nonzero(dst == 0) == N
    assert sorted(pos[dst == 0].tolist()) == list(range(N))                # a permutation ...
    assert not np.array_equal(pos[dst == 0], np.arange(N))                 # ... and not the identity
    lone = int(np.flatnonzero(dst == 1)[0])
    assert 0 < lone < N and lone % 64 and 0 <= pos[lone] < N               # the lone term sits inside a tile of 64
    again = sw.pack_targets(2403)["shared"]
    assert np.array_equal(again[0], dst) and np.array_equal(again[1], pos)
    assert sw.PACK_ROWS == 7 and (N + 1) % sw.PACK_ROWS and 64 % sw.PACK_ROWS
