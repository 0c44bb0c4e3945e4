"""CPU tests of TLWE packing: the library exports the entry points, the checker tests/pack_checker.py is
shown to be a key switch by decryption under a genuine key before the GPU tests compare words with it, the refusals that need no
device work, and the launch shapes of plan::plan_pack (cufhe_amd/csrc/launch_plan.h) through tests/host/plan_pack_harness.cpp."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import pack_checker as pk

n, N = ol.n, ol.N
NEW_SYMBOLS = ("cufhe_amd_pack_get_params", "cufhe_amd_pack_initialize", "cufhe_amd_pack_batch")
HARNESS_SRC = os.path.join(ol.ROOT, "tests", "host", "plan_pack_harness.cpp")
HARNESS = os.path.join(ol.ROOT, "tests", "host", "plan_pack_harness")
HARNESS_DEPS = [HARNESS_SRC, os.path.join(ol.ROOT, "cufhe_amd", "csrc", "launch_plan.h")]
PLAN_COUNTS = (1, 3, 64, 65, 130, 4096)
PLAN_CUS = (40, 104, 256)
TILE, CHUNKS, MAX_SLICES = 64, 8, (n + 15) // 16         # kPackTile, kPackChunks, ceil(n / kPackIBlock): kernels_pack.hip.h


def test_library_exports_the_new_entry_points():
    import cufhe_amd._lib as _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ol.ROOT, "include", "cufhe_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    import cufhe_amd.api as api
    p = api.pack_params()
    assert (p.n, p.N, p.t, p.basebit, p.key_words) == (n, N, pk.T, pk.BASEBIT, pk.KEY_WORDS) and pk.KEY_WORDS == 30965760
    for name in ("pack_params", "pack_initialize", "pack_batch", "gPackTLWEs"):
        assert callable(getattr(api, name))


def test_edge_words_have_the_digits_they_are_named_for():
    x = np.array(pk.EDGE_WORDS + (0,), np.uint32)
    d = pk.digits(x, rows=len(pk.EDGE_WORDS))
    assert not d[0].any() and not d[1].any()                 # 0 and 0x7FFF: below the rounding boundary
    assert list(d[2]) == [0] * 7 + [1]                      # 0x8000: rounds up into the last digit
    assert list(d[3]) == [3] * 8 and not d[4].any()          # 0xFFFF7FFF: all 3; 0xFFFF8000: the carry wraps to all-zero digits
    assert not d[5].any() and list(d[6]) == [3] * 8 and list(d[7]) == [3] * 8


def test_rotation_is_the_negacyclic_product():
    rng = np.random.default_rng(20)
    c = rng.integers(0, 1 << 32, size=2 * N, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(pk.rotate(c, 0), c)
    for e in (1, 511, 1023):
        r = pk.rotate(c, e).reshape(2, N)
        for p in range(2):
            for k in (0, 1, N - e - 1, N - e, N - 1):
                want = int(c[p * N + k]) if k + e < N else (-int(c[p * N + k])) % (1 << 32)
                assert int(r[p, (k + e) % N]) == want


def test_checker_decrypts_under_a_genuine_key(keys):
    """The full key: all n t 3 = 15 120 rows are built (a second or two: orc_polymul_ntt on threads), nothing is truncated.  12 lvl0
    encryptions go to three outputs -- one with a single input at 0, one with eight inputs at 0 .. 7, one with three at 1, 511, 1023 --
    and a fourth output stays unnamed.  The phase at coefficient pos[m] equals the phase of input m, and every other coefficient has
    phase 0, within 6 sigma of the derived error:
        rounding   a_i - sum_j a_ij 2^(32 - 2 (j+1)) is uniform in +-2^15 / 2^32 = +-2^-17 for each of the n / 2 secret bits that are 1:
                   variance (n / 2) 2^-34 / 3;
        key noise  at most n t rows of sigma 2^-25 per input: variance n t 2^-50
    so sigma^2 = (n / 2) 2^-34 / 3 + n t 2^-50, 6 sigma = 4.7e-4 ~ 2^-11, far inside the 1/8 margin of a gate input.  (The rows of the
    other inputs of an output add their key noise at every coefficient: 8 inputs raise the variance by 0.5 %; the bound asserted is
    the single-input one.)"""
    key = pk.genuine_key(keys, seed=31)
    assert key.size == pk.KEY_WORDS
    rng = np.random.default_rng(32)
    bits = rng.integers(0, 2, size=12).astype(np.uint8)
    ins = keys.encrypt(bits, 0, seed=33)
    dst = np.array([0] + [1] * 8 + [2] * 3, np.int32)
    pos = np.array([0] + list(range(8)) + [1, 511, 1023], np.int32)
    out = pk.pack_batch(key, ins, dst, pos, 4)
    sigma = np.sqrt((n / 2) * 2.0 ** -34 / 3 + n * pk.T * pk.KEY_SIGMA ** 2)
    bound = 6 * sigma * 2.0 ** 32
    assert 2.0 ** -12 < 6 * sigma < 2.0 ** -10
    assert not out[3].any()
    worst = 0
    for o in range(3):
        want = np.zeros(N, np.int64)
        for m in np.flatnonzero(dst == o):
            want[pos[m]] = pk.tlwe0_phase(keys, ins[m])
        err = np.abs(pk.signed(pk.trlwe_phase(keys, out[o]).astype(np.int64) - want))
        worst = max(worst, int(err.max()))
        assert err.max() < bound, (o, int(err.argmax()), int(err.max()), bound)
    print(f"max phase error {worst / 2.0 ** 32:.3e} of the torus, bound {6 * sigma:.3e}")
    # and the packed bits decrypt: the sign of the phase at pos[m] is the bit
    ph = [pk.signed(pk.trlwe_phase(keys, out[int(dst[m])]).astype(np.int64))[pos[m]] for m in range(12)]
    assert [int(p > 0) for p in ph] == list(bits)


def test_two_inputs_at_one_position_add(keys):
    rng = np.random.default_rng(40)
    key = rng.integers(0, 1 << 32, size=pk.KEY_WORDS, dtype=np.uint64).astype(np.uint32)
    x = pk.edge_inputs(rng, 2)
    one = pk.pack_batch(key, x, [0, 1], [5, 5], 2)
    both = pk.pack_batch(key, x, [0, 0], [5, 5], 1)
    assert np.array_equal(both[0], one[0] + one[1])


def test_refusals_that_need_no_device_work():
    import cufhe_amd._lib as _lib
    lib = _lib.lib
    fake = ctypes.c_void_p(4096)                             # never dereferenced: every call is refused before any device work
    ok = np.zeros(3, np.int32)

    def refused(rc, *words):
        msg = lib.cufhe_amd_last_error()
        assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)

    word = np.zeros(1, np.uint32)
    refused(lib.cufhe_amd_pack_initialize(None, pk.KEY_WORDS), b"null")
    refused(lib.cufhe_amd_pack_initialize(word.ctypes.data, 1), b"wrong size")
    refused(lib.cufhe_amd_pack_initialize(word.ctypes.data, pk.KEY_WORDS - 1), b"wrong size")
    refused(lib.cufhe_amd_pack_get_params(None), b"null")
    for args in ((None, ok.ctypes.data, ok.ctypes.data, fake), (fake, None, ok.ctypes.data, fake), (fake, ok.ctypes.data, None, fake),
                 (fake, ok.ctypes.data, ok.ctypes.data, None)):
        refused(lib.cufhe_amd_pack_batch(0, None, 3, args[0], args[1], args[2], 2, args[3]), b"null")
    for bad in (-1, 2):
        d = ok.copy()
        d[2] = bad
        refused(lib.cufhe_amd_pack_batch(0, None, 3, fake, d.ctypes.data, ok.ctypes.data, 2, fake), b"dst")
    for bad in (-1, N):
        p = ok.copy()
        p[0] = bad
        refused(lib.cufhe_amd_pack_batch(0, None, 3, fake, ok.ctypes.data, p.ctypes.data, 2, fake), b"pos")
    refused(lib.cufhe_amd_pack_batch(0, None, 3, fake, ok.ctypes.data, ok.ctypes.data, 0, fake), b"dst")
    # (well-formed arguments without a key, -3: tests/test_gpu_pack.py, with real device buffers)


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(HARNESS) or os.path.getmtime(HARNESS) < max(os.path.getmtime(d) for d in HARNESS_DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", HARNESS, HARNESS_SRC])
    return HARNESS


def plans(exe, requests):
    """[(count, cus, forced)] -> [(plan dict, workgroup rows [[chunk, tile, slice, first, inputs, i_begin, i_end]])]"""
    out = subprocess.run([exe], input="".join("%d %d %d\n" % r for r in requests), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    res = []
    for line in out.stdout.splitlines():
        f = line.split()
        if f[0] == "plan":
            res.append((dict(count=int(f[1]), cus=int(f[2]), forced=int(f[3]), tiles=int(f[5]), slices=int(f[7]), grid=(int(f[9]), int(f[10])),
                             max_slices=int(f[12])), []))
        else:
            res[-1][1].append([int(v) for v in f[1:]])
    assert len(res) == len(requests)
    return res


def check_cover(p, wgs):
    count = p["count"]
    assert p["slices"] >= 1 and p["slices"] <= p["max_slices"] == MAX_SLICES
    assert p["tiles"] == (count + TILE - 1) // TILE
    assert p["grid"] == (CHUNKS * p["tiles"], p["slices"]) and len(wgs) == p["grid"][0] * p["grid"][1]
    cover = np.zeros((CHUNKS, count, n), np.int32)
    for c, tile, sl, first, inputs, i0, i1 in wgs:
        assert 0 <= c < CHUNKS and 0 <= tile < p["tiles"] and 0 <= sl < p["slices"]
        assert 1 <= inputs <= TILE and 0 <= first and first + inputs <= count and 0 <= i0 <= i1 <= n
        cover[c, first:first + inputs, i0:i1] += 1
    assert (cover == 1).all(), "an (input, i) pair of a chunk is covered %d .. %d times" % (cover.min(), cover.max())
    # the b word is added by slice 0 of the chunk that holds row word N: there is exactly one such workgroup per tile
    assert sorted(w[1] for w in wgs if w[0] == N // 256 and w[2] == 0) == list(range(p["tiles"]))


def test_plan_pack_covers_every_input_and_every_i_once(harness):
    reqs = [(count, cus, -1) for count in PLAN_COUNTS for cus in PLAN_CUS]
    for p, wgs in plans(harness, reqs):
        check_cover(p, wgs)
    got = {(p["count"], p["cus"]): p["slices"] for p, _ in plans(harness, reqs)}
    # the rule: four workgroups per CU wanted, 8 per tile given, at most ceil(n / 16) slices
    for (count, cus), slices in got.items():
        wg = CHUNKS * ((count + TILE - 1) // TILE)
        assert slices == (1 if wg >= 4 * cus else min(MAX_SLICES, -(-4 * cus // wg))), (count, cus, slices)
    assert got[(4096, 40)] == 1 and got[(1, 256)] == MAX_SLICES


def test_plan_pack_forced_slices(harness):
    """"pack_slices": any value is clamped to 1 .. max; slice counts that do not divide n leave the last slices empty, never overlapping"""
    reqs = [(count, 256, forced) for count in (1, 65, 130) for forced in (1, 2, 3, 7, 37, 39, 40, 41, 1000)]
    for p, wgs in plans(harness, reqs):
        assert p["slices"] == min(p["forced"], MAX_SLICES)
        check_cover(p, wgs)


def test_cpp_program_compiles():
    """tests/cpp/test_pack.cpp builds against include/cufhe_amd.hpp, the library and the oracle (it runs in the GPU suite)"""
    assert os.path.exists(pk.build_cpp_program())
