"""Whole argument domains of the two index-arithmetic kernel families the exponent sweep leaves out: helpers of
tests/test_argument_sweeps.py and tests/test_gpu_argument_sweeps.py.  numpy only: no GPU, no kernel code.

Spread (cufhe_amd_trlwe_spread_batch, kernels_lut.hip.h) takes any stride >= 1, reps >= 1 with stride reps <= N: 7262 pairs.
`spread_all` is the defining sum evaluated incrementally over ALL of them -- with chat the 2N negacyclic extension of a polynomial,
    U_r = U_(r-1) + roll(chat, (r - 1) stride)  mod 2^32,        W[k] = U_r[k + stride (r // 2)],   k < N
-- one roll and one add per pair, nothing shared with the kernel's class-major prefix sum.  tests/test_argument_sweeps.py pins it
to lut_checker.spread (one term at a time) before the GPU tests compare words with it.

Packing (cufhe_amd_pack_batch / cufhe_amd_enqueue_pack, kernels_pack.hip.h) applies X^pos at the atomic write-out, pos in [0, N),
and takes up to N terms per recorded node: `pack_targets` gives the dst / pos lists that meet every position, alone and all in one
output."""
import numpy as np

N = 1024
M32 = 0xFFFFFFFF
SPREAD_PAIRS = 7262                                       # sum_{s = 1 .. N} floor(N / s)
EDGE_WORDS = (0x00000000, 0x00000001, 0x80000000, 0xFFFFFFFF)
# the pairs the suite ran before this sweep (SPREADS of tests/test_gpu_lut.py and tests/footprint.py)
EXISTING_SPREADS = ((1, 1), (1, 2), (1, 3), (1, 256), (1, 1024), (4, 64), (8, 128), (3, 341))
# stride bands of at most 1304 pairs (32 MB of output at 3 TRLWEs per pair), together all strides
SPREAD_BANDS = ((1, 1), (2, 3), (4, 7), (8, 15), (16, 56), (57, 215), (216, 1024))
PACK_ROWS = 7                                             # distinct lvl0 inputs of the packing sweeps (a period of tests/positions.py)


def spread_pairs(strides=None):
    """every (stride, reps) the batch call accepts, stride rising, reps rising within a stride: the order of spread_all"""
    strides = range(1, N + 1) if strides is None else strides
    return [(s, r) for s in strides for r in range(1, N // s + 1)]


def recorded_spread_pairs():
    """the 66 pairs the recorded form takes: stride = 2^a, reps = 2^b, a + b <= 10"""
    return [(1 << a, 1 << b) for a in range(11) for b in range(11 - a)]


def spread_all(c, strides=None):
    """yields ((stride, reps), W) over spread_pairs(strides) for c of shape [polys][N] uint32; W [polys][N] is a fresh array"""
    c = np.ascontiguousarray(c, np.uint32)
    assert c.ndim == 2 and c.shape[1] == N
    chat = np.concatenate([c, np.uint32(0) - c], axis=1)                  # chat[m + N] = -chat[m]
    for stride in (range(1, N + 1) if strides is None else strides):
        u = np.zeros_like(chat)
        for reps in range(1, N // stride + 1):
            u += np.roll(chat, (reps - 1) * stride, axis=1)               # rolled[m] = chat[m - (reps - 1) stride]; uint32 wraps
            first = stride * (reps // 2)
            yield (stride, reps), u[:, first:first + N].copy()


def sweep_inputs(seed):
    """[3][2N] uint32: two TRLWEs of full-range random words with the EDGE_WORDS sown in at 64 random coefficients each, and the
    "delta" TRLWE -- polynomial a the word 1 at coefficient 0, polynomial b the word 0xFFFFFFFF at coefficient N - 1 -- whose Spread
    is the window's +-1 mask"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 1 << 32, size=(3, 2 * N), dtype=np.uint64).astype(np.uint32)
    for g in range(2):
        at = rng.choice(2 * N, size=64, replace=False)
        x[g, at] = np.array(EDGE_WORDS, np.uint32)[np.arange(64) % len(EDGE_WORDS)]
    x[2] = 0
    x[2, 0] = 1
    x[2, 2 * N - 1] = M32
    return x


def delta_window(stride, reps, at, word):
    """[N] uint32: Spread of the polynomial `word` X^at, from the exponents i stride - stride (reps // 2) themselves"""
    e = (at + np.arange(reps, dtype=np.int64) * stride - stride * (reps // 2)) % (2 * N)
    out = np.zeros(N, np.uint32)
    out[e % N] = np.where(e >= N, (0 - int(word)) & M32, int(word)).astype(np.uint32)
    return out


def recorded_spread_order(seed):
    """the 66 recorded pairs in a seeded order in which neighbouring records differ in BOTH stride and reps, so that the two TRLWEs of
    one workgroup of trlwe_spread_desc_kernel (records 2 i and 2 i + 1) never share a descriptor's numbers"""
    pairs = recorded_spread_pairs()
    rng = np.random.default_rng(seed)
    rest = [pairs[i] for i in rng.permutation(len(pairs))]
    apart = lambda p, q: p[0] != q[0] and p[1] != q[1]
    order = [rest.pop(0)]
    while rest:
        fit = next((i for i, p in enumerate(rest) if apart(order[-1], p)), None)
        if fit is not None:
            order.append(rest.pop(fit))
            continue
        p = rest.pop(0)                                   # nothing left follows the tail: put p between two records it differs from
        at = next(i for i in range(1, len(order)) if apart(order[i - 1], p) and apart(p, order[i]))
        order.insert(at, p)
    assert sorted(order) == sorted(pairs) and all(apart(order[i], order[i + 1]) for i in range(len(order) - 1))
    return order


def pack_targets(seed, count=N + 1):
    """the dst / pos lists of the packing sweep over `count` = N + 1 inputs, {name: (dst, pos, count_out)}:
         "isolated"  dst[m] = m, pos[m] = m mod N: every position alone in an output of its own
         "shared"    output 0 receives N terms whose positions are a seeded permutation of 0 .. N - 1, output 1 the remaining term (a
                     seeded input inside a tile, at a seeded position)"""
    assert count == N + 1
    rng = np.random.default_rng(seed)
    m = np.arange(count)
    lone = 64 * int(rng.integers(0, N // 64)) + int(rng.integers(1, 64))
    dst = np.zeros(count, np.int32)
    dst[lone] = 1
    pos = np.empty(count, np.int32)
    pos[m != lone] = rng.permutation(N)
    pos[lone] = int(rng.integers(0, N))
    return {"isolated": (m.astype(np.int32), (m % N).astype(np.int32), count), "shared": (dst, pos, 2)}


def schoolbook_rotate(row, e):
    """X^e times both polynomials of a TRLWE row by schoolbook multiplication mod X^N + 1, 2^32: the product with the monomial, term
    by term through the 2N - 1 coefficients of the plain product"""
    c = np.ascontiguousarray(row, np.uint32).reshape(2, N).astype(np.int64)
    mono = np.zeros(N, np.int64)
    mono[e] = 1
    out = np.empty((2, N), np.uint32)
    for j in range(2):
        full = np.convolve(c[j], mono)                                    # 2N - 1 coefficients, each one input word: no overflow
        red = full[:N].copy()
        red[:N - 1] -= full[N:]
        out[j] = (red & M32).astype(np.uint32)
    return out.reshape(2 * N)


def describe_spread_failure(stride, reps, poly, k):
    """a wrong word of Spread at coefficient k of polynomial `poly` in the terms of trlwe_spread_wave (kernels_lut.hip.h): where the
    window lies in the class-major order and which of the two branches forms it"""
    length, shift = N // stride, stride * (reps // 2)
    big = N - length * stride
    split = big * (length + 1)
    start_of = lambda rho: rho * (length + 1) if rho < big else split + (rho - big) * length
    neg = k + shift >= N
    m = k + shift - N if neg else k + shift
    t = m // stride
    rho = m - t * stride
    q = start_of(rho) + t
    text = (f"(stride, reps) = ({stride}, {reps}), polynomial {poly} (TRLWE {poly // 2}, wave {poly % 4} of its workgroup), coefficient {k} "
            f"(lane {k % 64}, register {k // 64}): m = {m}{' (negated: k + shift >= N)' if neg else ''}, rho = {rho}, t = {t}, "
            f"len = {length}, big = {big}, split = {split}, class of {length + 1 if rho < big else length} members from position "
            f"{start_of(rho)}, q = {q}; ")
    if t >= reps:
        return text + f"branch t >= reps: pre[{q + 1}] - pre[{q + 1 - reps}]"
    jmax = N - stride + rho
    tj = jmax // stride
    qj = start_of(jmax - tj * stride) + tj
    return text + (f"branch t < reps (negacyclic wrap): pre[{q + 1}] - pre[{start_of(rho)}] - (pre[{qj + 1}] - pre[{qj + 1 - (reps - 1 - t)}]), "
                   f"jmax = {jmax}, qj = {qj}, {reps - 1 - t} members of the class of m + N")
