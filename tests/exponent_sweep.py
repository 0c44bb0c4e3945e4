"""The exponent axis of every rotating kernel, restated from the definitions of include/cufhe_amd.h in plain Python integers and
numpy: the modulus switch and the words at both ends of each of its rounding intervals, X^e p in Z_{2^w}[X]/(X^N + 1), the
accumulator a blind rotation starts from, and SampleExtract(j).  Parameterised by the ring (N = 2^nbit, k mask polynomials) and the
torus width (32 or 64 bits).  Nothing here is shared with the kernels or with the other checkers of tests/: tests/test_exponent_sweep.py
pins this file against all of them, exponent by exponent, before tests/test_gpu_exponent_sweep.py compares kernels with it.

    abar = (((a + 2^(30 - nbit + s)) mod 2^32) >> (31 - nbit + s)) << s         rounds;  2N wraps to 0
    bbar = 2N - ((b >> (31 - nbit + s)) << s)                                   truncates;  b in the first interval gives 2N
    X^e X^i = X^(i + e),  X^N = -1                                               0 <= e <= 2N
    SampleExtract(j): out[c N + m] = a_c[j - m] (m <= j), -a_c[N + j - m] (m > j);  out[k N] = b[j]
"""
from collections import namedtuple

import numpy as np

M32 = 0xFFFFFFFF
DTYPE = {32: np.uint32, 64: np.uint64}

Edges = namedtuple("Edges", "t a bbar b")


def ms_abar(a, nbit, s=0):
    sh = 31 - nbit + s
    return ((((int(a) & M32) + (1 << (sh - 1))) & M32) >> sh) << s


def ms_bbar(b, nbit, s=0):
    return (2 << nbit) - (((int(b) & M32) >> (31 - nbit + s)) << s)


def edge_words(nbit, s=0):
    """Edges(t, a, bbar, b): t the grid of exponents (multiples of 2^s in [0, 2N), ascending); a[i] = (smallest, largest) 32-bit word
    whose abar is t[i] -- the interval of t = 0 begins just below 2^32 and ends above 0, so its `smallest` is its first word in
    cyclic order; bbar[i] = 2N - t[i] (2N for i = 0) and b[i] = (smallest, largest) word whose bbar is bbar[i]"""
    sh = 31 - nbit + s
    width, half = 1 << sh, 1 << (sh - 1)
    t = np.arange(0, 2 << nbit, 1 << s, dtype=np.int64)
    q = t >> s
    a = np.stack([(q * width - half) % (1 << 32), (q * width + width - half - 1) % (1 << 32)], axis=1)
    b = np.stack([q * width, q * width + width - 1], axis=1)
    return Edges(t, a.astype(np.uint32), (2 << nbit) - t, b.astype(np.uint32))


def rotate(poly, e, N=None):
    """X^e poly in Z_{2^w}[X]/(X^N + 1), 0 <= e <= 2N, w the width of poly's dtype: term i moves to i + e, and every pass over X^N
    changes its sign"""
    poly = np.asarray(poly)
    N = poly.size if N is None else N
    assert poly.shape == (N,) and 0 <= e <= 2 * N and poly.dtype in (np.uint32, np.uint64)
    out = np.zeros_like(poly)
    neg = (~poly) + poly.dtype.type(1)                       # -p mod 2^w
    for i in range(N):
        d = i + int(e)
        passes, pos = divmod(d, N)
        out[pos] = neg[i] if passes & 1 else poly[i]
    return out


def rotate_many(polys, e, N):
    """rotate() of every row of polys[..., N] by the same e: the same scatter, all terms i at once"""
    polys = np.asarray(polys)
    d = np.arange(N) + int(e)
    out = np.empty_like(polys)
    neg = (~polys) + polys.dtype.type(1)
    out[..., d % N] = np.where((d // N) & 1 == 1, neg, polys)
    return out


def start_acc(kind, bword, s, nbit, k=1, bits=32, tv=None, table=None, const=None):
    """the accumulator ((k + 1) N words of `bits` bits) a blind rotation of a ciphertext with last word `bword` holds after 0 steps:
        "mu"     (0, .., 0, X^bbar mu),  mu = 2^(bits - 3) in every coefficient: the built-in gates
        "const"  the same with `const` in every coefficient
        "tv"     (0, .., 0, X^bbar tv): a user gate's row
        "table"  X^bbar on each of the k + 1 polynomials of a caller's TRLWE `table`"""
    N, dt = 1 << nbit, DTYPE[bits]
    bbar = ms_bbar(bword, nbit, s)
    if kind == "table":
        return rotate_many(np.asarray(table, dt).reshape(k + 1, N), bbar, N).reshape(-1)
    if kind == "mu":
        last = np.full(N, 1 << (bits - 3), dt)
    elif kind == "const":
        last = np.full(N, const, dt)
    elif kind == "tv":
        last = np.asarray(tv, dt).reshape(N)
    else:
        raise ValueError(kind)
    acc = np.zeros((k + 1) * N, dt)
    acc[k * N:] = rotate_many(last, bbar, N)
    return acc


def extract(acc, j, N, k=1):
    """SampleExtract(j) of an accumulator of (k + 1) N words: the TLWE of k N + 1 words of coefficient j"""
    acc = np.asarray(acc)
    assert acc.shape == ((k + 1) * N,) and 0 <= j < N
    out = np.empty(k * N + 1, acc.dtype)
    one = acc.dtype.type(1)
    m = np.arange(N)
    low = m <= j                                             # the two branches of the definition, each on its own m
    for c in range(k):
        a = acc[c * N:(c + 1) * N]
        out[c * N + m[low]] = a[j - m[low]]
        out[c * N + m[~low]] = (~a[N + j - m[~low]]) + one
    out[k * N] = acc[k * N + j]
    return out


def sweep_rows(edges, which, n, rng, fixed=None):
    """lvl0 ciphertexts [2 T + 1][n + 1] of random words that carry every exponent: row g holds edge g % 2 of exponent index g // 2 in
    word 0 (which = "a") or in the last word (which = "b"); the last row is random throughout (an odd count).  fixed: {word: value}
    put into every row but the last afterwards"""
    T = edges.t.size
    rows = rng.integers(0, 1 << 32, size=(2 * T + 1, n + 1), dtype=np.uint64).astype(np.uint32)
    src = edges.a if which == "a" else edges.b
    rows[:2 * T, 0 if which == "a" else n] = src.reshape(-1)
    for w, v in (fixed or {}).items():
        rows[:2 * T, w] = v
    return rows


def describe(got, want, edges, which):
    """None if equal, else the count of bad rows and the first bad exponent, edge and word"""
    got, want = np.asarray(got).reshape(want.shape[0], -1), want.reshape(want.shape[0], -1)
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size == 0:
        return None
    g = int(bad[0])
    w = int(np.flatnonzero(got[g] != want[g])[0])
    T = edges.t.size
    where = "the extra random row" if g >= 2 * T else "%sbar %d, %s edge" % (
        which, int(edges.t[g // 2] if which == "a" else edges.bbar[g // 2]), ("low", "high")[g % 2])
    return "%d of %d rows differ; first: row %d (%s), word %d: got %#x, want %#x" % (bad.size, want.shape[0], g, where, w, int(got[g, w]), int(want[g, w]))
