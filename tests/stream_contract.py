"""The stream contract of the batch entry points: host-only helpers of tests/test_gpu_stream_contract.py (tests/test_stream_contract.py
checks them on the CPU).

Three things are decided here, away from the device, so that they can be checked without one:

  * which counts make the grow-only pools regrow in the middle of a chain (`grows`): the stream's workspace (open_scratch: a block of
    need + need / 4 + 1 MiB, freed and replaced when a later call needs more), the digit words of the matrix key switch (ks_digits:
    the exact size, freed and replaced when a later launch has more tiles) and the temporary of cufhe_amd_linear_gate_batch
    (g_linear_tmp: the exact size);
  * the order in which several lanes (one stream each) issue their calls from one thread (`round_robin`);
  * the OTHER VALID values a host argument array is overwritten with once its call has returned (`other_*`): defined ops of the same
    arity, in-range exponents, indices and positions -- a late read gives a wrong word, never a wild pointer -- and, as the CPU-side
    proof that a late read would be seen, `differs_in_every_row`.
"""
import numpy as np

W0, W1 = 631, 1025                  # words of a lvl0 / lvl1 ciphertext of the default set
N = 1024
LIN_DESC = 40                       # sizeof(LinDesc): three pointers, ca, cb, off, pad (kernels_common.hip.h)
MIB = 1 << 20
KS_MM_ROWS = 64                     # kKsMmRows; tests/test_gpu_stream_contract.py asserts it is the library's
KS_MM_TILE_BYTES = 512 * 64 * 4     # ks_mm_digit_bytes of one tile: kKsMmSteps (N / 2 = 512) steps of 64 digit words

# Counts of the gate chain.  A two-input gate needs a lvl1 and a lvl0 temporary and six descriptors (run_gates, capi.hip):
#     need(c) = c (1025 * 4 + 631 * 4 + 6 * 40) + 8 * 40 + 8192 = 6864 c + 8512 bytes
# and open_scratch allocates A(c) = need(c) + need(c) / 4 + 2^20.  A fourfold step regrows when need(4 c) > A(c):
#     27456 c + 8512 > 8580 c + 10640 + 1048576   <=>   c >= 56,
# so 8 -> 1024 regrows (7 037 248 > A(8) = 1 127 856), 1024 -> 8 reuses the block shrunk, 8 -> 4096 regrows again (28 123 456 >
# A(1024) = 9 845 136) and 4096 -> 9 reuses it.
GATE_COUNTS = (8, 1024, 8, 4096, 9)
# the same fall and rise at sizes that keep a pair of lanes, or a lane on the workgroup-per-rotation kernels, short:
# need(300) = 2 067 712 > A(8), need(1300) = 8 931 712 > A(300) = 3 633 216
SHORT_COUNTS = (8, 300, 8, 1300, 9)
# key switches: one tile with one live row, a second tile, back, four times as many tiles
KS_COUNTS = (1, KS_MM_ROWS + 1, 1, 4 * (KS_MM_ROWS + 1))


def gate_need(count, rotations_per_gate=1):
    """bytes run_gates asks open_scratch for: `count` gates of the default set without multi-output or three-input user gates"""
    return count * rotations_per_gate * (W1 * 4 + W0 * 4) + (count * 6 + 8) * LIN_DESC + 8192


def grows(needs, slack=True):
    """[bool per call]: the pool is freed and replaced (True) or reused (False); the first call allocates (True).  slack: the workspace
    (a quarter plus 1 MiB on top of the need); False: ks_digits and g_linear_tmp, which allocate the exact size."""
    have, out = 0, []
    for need in needs:
        out.append(have < need)
        if have < need:
            have = need + need // 4 + MIB if slack else need
    return out


def ks_digit_bytes(count):
    return (count + KS_MM_ROWS - 1) // KS_MM_ROWS * KS_MM_TILE_BYTES


def round_robin(lengths):
    """[(lane, call)]: A1 B1 A2 B2 ... for lanes of the given numbers of calls; a shorter lane simply ends earlier"""
    return [(lane, i) for i in range(max(lengths, default=0)) for lane, n in enumerate(lengths) if i < n]


# ---- other valid values ----
TWO_INPUT_OPS = 10                  # ops 0 .. 9 read two operands (include/cufhe_amd.h)


def other_ops(ops):
    """another built-in op of the same arity for every entry: two-input ops move on by one, MUX <-> NMUX, NOT <-> COPY"""
    ops = np.asarray(ops, np.int32)
    out = np.where(ops < TWO_INPUT_OPS, (ops + 1) % TWO_INPUT_OPS, np.where(ops < 12, 21 - ops, 25 - ops)).astype(np.int32)
    assert ((out >= 0) & (out < 14) & (out != ops)).all()
    return out


def other_in_range(values, bound, step):
    """(v + step) mod bound: in [0, bound), different from v in every entry"""
    values = np.asarray(values, np.int32)
    assert 0 < step < bound and ((values >= 0) & (values < bound)).all()
    return ((values.astype(np.int64) + step) % bound).astype(np.int32)


def differs_in_every_row(a, b):
    """no row of `a` equals the same row of `b`: a call that ran on the overwritten arguments would fail the comparison in every row"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((a.reshape(a.shape[0], -1) != b.reshape(b.shape[0], -1)).any(axis=1).all())
