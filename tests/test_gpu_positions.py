"""Every output word at every batch position, on every launch shape (tests/positions.py).

Each path builds its batches from D distinct inputs (positions.PATHS), row g carrying input g % D: the reference is computed once
per (path, level) for the D inputs, on threads, and ALL rows of every launch are compared with it, word for word, after the output
buffer was filled with 0xDEADBEEF.  The distinct cases cycle through all 14 ops (MUX / NMUX cost two rotations, NOT / COPY none:
the rotation index is not the gate index) and carry the corner inputs of test_gpu_parity.py::test_blind_rotate_accumulator_words
(a run of abar = 0; bbar = 2N, 1, N; words 0x7FFFFFFF).  No comparison here indexes the result with a subset of rows.
"""
import ctypes
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as ol
import positions as pos

pytestmark = pytest.mark.gpu

D = pos.D_ORACLE
DC = pos.D_CHECKER
THREADS = min(16, os.cpu_count() or 1)
SHAPES = {   # the four forced shapes of test_gpu_parity.py's br_kernel fixture, with the key-switch shape each selects
    "batch": dict(ll2_threshold=0, ll_threshold=0, half_threshold=0, ks_wg_threshold=0, ks_split_threshold=0),
    "half": dict(ll2_threshold=0, ll_threshold=0, half_threshold=1 << 30, ks_wg_threshold=0, ks_split_threshold=0),
    "ll": dict(ll2_threshold=0, ll_threshold=1 << 30, half_threshold=0, ks_wg_threshold=1 << 30, ks_split_threshold=1 << 30),
    "ll2": dict(ll2_threshold=1 << 30, ll_threshold=0, half_threshold=0, ks_wg_threshold=1 << 30, ks_split_threshold=0),
}
COUNTS = [1, 7, 8, 9, 15, 16, 17, 129, 255, 256, 257, 300, 511, 513, 600, 700, 1031, 1100, 1300, 1536, 2047, 2048, 2049, 2700, 3200,
          3500, 4096, 4600]
U32 = lambda rng, shape: rng.integers(0, 2**32, size=shape, dtype=np.uint64).astype(np.uint32)  # noqa: E731


def _pmap(fn, items):
    """fn over items on threads (ctypes releases the GIL); the first one alone, so that the oracle builds its tables once"""
    items = list(items)
    first = [fn(items[0])]
    with ThreadPoolExecutor(THREADS) as ex:
        return first + list(ex.map(fn, items[1:]))


def _up(eng, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.uint32)
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return eng.api.DeviceBuffer(a.size).upload(a)


def _groupings(eng):
    c = eng.api.device_cus()
    return (4, 8, 12, 16, 2 * c, 8 * c)


def _corner_tlwe0(rng, n_, count):
    """lvl0 ciphertexts of random words with the corner inputs of test_blind_rotate_accumulator_words in rows 0 .. 4"""
    tl = U32(rng, (count, n_ + 1))
    tl[0, :4] = 0                                  # a run of abar = 0
    tl[1, n_] = 0                                  # bbar = 2N
    tl[2, n_] = 0xFFFFFFFF                         # bbar = 1
    tl[3, :8] = 0x7FFFFFFF
    tl[3, n_] = 0x80000000                         # bbar = N
    tl[4, :] = 0x7FFFFFFF
    return tl


class Gates:
    """The D distinct gates of one (path, level): ops i % 14 on encryptions of random bits; the NAND cases (i = 0, 14, 28, 42, 56)
    carry the corner inputs -- at level 0 the combination (0, mu) - in0 - in1 that enters the blind rotation has a run of zero
    words, b = 0 (bbar = 2N), b = -1 (bbar = 1), b = 2^31 (bbar = N) with words 0x7FFFFFFF, and all words 0x7FFFFFFF on both
    inputs; at level 1 the same words meet the key switch first.  `reference(ops, in0, in1, in2)` gives the expected words."""

    def __init__(self, eng, K, level, mu, reference, seed, largest):
        self.level, self.words = level, K.words[level]
        rng = np.random.default_rng(seed)
        bits = rng.integers(0, 2, size=(3, D)).astype(np.uint8)
        ins = [K.encrypt(bits[i], level, seed=seed + 1 + i) for i in range(3)]
        w = self.words - 1
        ins[0][0, :4] = 0; ins[1][0, :4] = 0
        ins[0][14, w] = mu; ins[1][14, w] = 0
        ins[0][28, w] = mu + 1; ins[1][28, w] = 0
        ins[0][42, :8] = 0x7FFFFFFF; ins[1][42, :8] = 0
        ins[0][42, w] = (mu - 0x80000000) & 0xFFFFFFFF; ins[1][42, w] = 0
        ins[0][56, :] = 0x7FFFFFFF; ins[1][56, :] = 0x7FFFFFFF
        self.ins = ins
        self.ops = (np.arange(D) % 14).astype(np.int32)
        t0 = time.time()
        self.want = reference(self.ops, *ins)
        self.want_mux = None
        self.reference = reference
        print(f"\n[positions] reference of {D} distinct gates, level {level}, {K.set_name}: {time.time() - t0:.2f} s")
        self.largest = largest
        self.t_ops = pos.tile(self.ops, largest)
        self.din = [_up(eng, pos.tile(x, largest)) for x in ins]
        self.dout = eng.api.DeviceBuffer(largest * self.words)

    def uniform(self, op):
        """the expected words when every gate runs `op` (ops_stride 0)"""
        return self.reference(np.full(D, op, np.int32), *self.ins)

    def run(self, launch, count):
        """poison the output, launch(ops, dout, din0, din1, din2, count), return all rows"""
        assert count <= self.largest
        self.dout.upload(pos.poison(count * self.words))
        launch(self.t_ops[:count], self.dout, self.din[0], self.din[1], self.din[2], count)
        return self.dout.download(count * self.words).reshape(count, self.words)


# ---------------------------------------------------------------------------------------------------------------------------------
# a. the default path, cufhe_amd_gate_batch
# ---------------------------------------------------------------------------------------------------------------------------------
_cache = {}       # the Gates of a (path, level), built on first use and shared by the fixtures of this module


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _cache.clear()


def _base(engine, keys, level):
    if ("base", level) not in _cache:
        _cache["base", level] = Gates(engine, keys, level, ol.MU, lambda ops, a, b, c: keys.gate_batch(ops, level, a, b, c), 9100 + 10 * level,
                                      32768 if level == 0 else 4600)
    return _cache["base", level]


@pytest.fixture(scope="module", params=[0, 1])
def base(request, engine, keys):
    return _base(engine, keys, request.param)


@pytest.fixture(scope="module")
def base0(engine, keys):
    """level 0 only: the BASELINE configs[2] size"""
    return _base(engine, keys, 0)


def _batch(eng, level):
    return lambda ops, out, a, b, c, count: eng.gate_batch(ops, level, out, a, b, c, count=count)


def _check(eng, G, count, label, opts=None, launch=None):
    with pos.options(eng.api, opts or {}):
        got = G.run(launch or _batch(eng, G.level), count)
        groupings = _groupings(eng)
    pos.assert_every_row(got, G.want, f"{label}, level {G.level}, {count} gates", groupings)


@pytest.mark.parametrize("count", COUNTS)
def test_default_rules(engine, base, count):
    _check(engine, base, count, "default launch rules")


def test_default_rules_32768(engine, base0):
    _check(engine, base0, 32768, "default launch rules")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_forced_shapes(engine, base, shape):
    for count in COUNTS:
        if count <= (300 if shape in ("ll", "ll2") else 1031):      # a workgroup per rotation: up to 300, as test_ragged_batch_sizes
            _check(engine, base, count, f"shape {shape}", SHAPES[shape])


@pytest.mark.parametrize("opts", [dict(ll_threshold=0, ll2_threshold=0), dict(ll2_threshold=0)], ids=["no-ll-no-ll2", "no-ll2"])
def test_tail_option_sets(engine, base, opts):
    """the option sets of test_launch_shapes_with_tails (the third one, no option, is test_default_rules), each at all three counts"""
    for count in (700, 1100, 3200):
        _check(engine, base, count, f"options {opts}", opts)


@pytest.mark.parametrize("per,slices", [(1, 1), (6, 1), (16, 2), (9, 4), (16, 64)])
def test_keyswitch_shapes(engine, base, per, slices):
    for count in (257, 1031):
        _check(engine, base, count, f"key switch {per} per workgroup, {slices} runs of j",
               dict(ks_wg_threshold=0, ks_split_threshold=0, ks_per_wg=per, ks_slices=slices))


@pytest.mark.parametrize("cus", [40, 104])
def test_other_cu_counts(engine, base, cus):
    for count in (8 * cus + cus + 3, 16 * cus + 1):
        _check(engine, base, count, f"cus_override {cus}", dict(cus_override=cus))


# ---------------------------------------------------------------------------------------------------------------------------------
# b. operand addressing: padded strides, ops_stride, aliasing, scattered operands
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [1, 5])
def test_padded_stride(engine, base, pad):
    """rows on odd word offsets: stride_words = words + pad; the pad words are poisoned before and unchanged after, in every buffer"""
    G, api = base, engine.api
    stride = G.words + pad
    for count in (17, 300, 2049):
        host = []
        for x in G.ins:
            h = pos.poison((count, stride))
            h[:, :G.words] = pos.tile(x, count)
            host.append(h)
        din = [_up(engine, h) for h in host]
        dout = _up(engine, pos.poison(count * stride))
        api.gate_batch(G.t_ops[:count], G.level, dout, din[0], din[1], din[2], count=count, stride_words=stride)
        got = dout.download().reshape(count, stride)
        pos.assert_every_row(np.ascontiguousarray(got[:, :G.words]), G.want, f"stride words + {pad}, level {G.level}, {count} gates", _groupings(engine))
        assert np.array_equal(got[:, G.words:], pos.poison((count, pad))), f"stride words + {pad}: the pad words of the output were written"
        for i in range(3):
            assert np.array_equal(din[i].download().reshape(count, stride), host[i]), f"stride words + {pad}: operand {i} was written"


@pytest.mark.parametrize("ops_stride", [0, 1, 2])
def test_ops_stride(engine, base, ops_stride):
    """ops[g * ops_stride]: 0 = ops[0] for all (the other entries hold a different, valid op that must not be used), 2 = every
    second entry"""
    G, api = base, engine.api
    for count in (17, 300, 2049):
        t = G.t_ops[:count]
        if ops_stride == 0:
            ops = np.concatenate([[api.MUX], (t[1:] + 1) % 14]).astype(np.int32)
            if G.want_mux is None:
                G.want_mux = G.uniform(api.MUX)
            want = G.want_mux
        elif ops_stride == 1:
            ops, want = t, G.want
        else:
            ops = np.stack([t, (t + 1) % 14], axis=1).ravel().astype(np.int32)
            want = G.want
        got = G.run(lambda _, out, a, b, c, n_: api.gate_batch(ops, G.level, out, a, b, c, count=n_, ops_stride=ops_stride), count)
        pos.assert_every_row(got, want, f"ops_stride {ops_stride}, level {G.level}, {count} gates", _groupings(engine))


def test_out_aliases_in0(engine, base):
    G = base
    for count in (17, 300, 2049):
        d0 = _up(engine, pos.tile(G.ins[0], count))
        engine.gate_batch(G.t_ops[:count], G.level, d0, d0, G.din[1], G.din[2], count=count)
        pos.assert_every_row(d0.download().reshape(count, G.words), G.want, f"out == in0, level {G.level}, {count} gates", _groupings(engine))


def test_gate_list_scattered_operands(engine, base):
    """cufhe_amd_gate_list: the rows of every operand and of the output scattered by a random permutation inside a larger buffer"""
    G, api = base, engine.api
    rng = np.random.default_rng(77 + G.level)
    for count in (17, 300, 2049):
        slots = count + 50
        perms = [rng.permutation(slots)[:count] for _ in range(4)]
        bufs = []
        for i in range(3):
            h = pos.poison((slots, G.words))
            h[perms[i]] = pos.tile(G.ins[i], count)
            bufs.append(_up(engine, h))
        dout = _up(engine, pos.poison(slots * G.words))
        arr = lambda d, p: (ctypes.c_void_p * count)(*[d.ptr + int(r) * G.words * 4 for r in p])  # noqa: E731
        ops = np.ascontiguousarray(G.t_ops[:count])
        engine.check(engine.lib.cufhe_amd_gate_list(0, None, G.level, count, ops.ctypes.data, arr(dout, perms[3]), arr(bufs[0], perms[0]),
                                                    arr(bufs[1], perms[1]), arr(bufs[2], perms[2])))
        out = dout.download().reshape(slots, G.words)
        pos.assert_every_row(np.ascontiguousarray(out[perms[3]]), G.want, f"gate_list scattered, level {G.level}, {count} gates", _groupings(engine))
        rest = np.setdiff1d(np.arange(slots), perms[3])
        assert np.array_equal(out[rest], pos.poison((rest.size, G.words))), "gate_list wrote a slot no gate names"


# ---------------------------------------------------------------------------------------------------------------------------------
# c. the per-gate API: 32 768 gates on 256 streams
# ---------------------------------------------------------------------------------------------------------------------------------
def test_per_gate_api_32768_on_256_streams(engine, base0):
    """the shape of test_config2_mixed_32768_per_gate_api_256_streams with the tiled set: every tlwehost row; again with
    "sched_zero_copy" 0 (staging through the copy engine)"""
    G, api = base0, engine.api
    count, nst = 32768, 256
    sts = [api.Stream() for _ in range(nst)]
    for s in sts:
        s.Create()
    tiled = [pos.tile(x, count) for x in G.ins]
    cin = [[api.Ctxt(0) for _ in range(count)] for _ in range(3)]
    for i in range(3):
        for g in range(count):
            cin[i][g].tlwehost[:] = tiled[i][g]
    outs = [api.Ctxt(0) for _ in range(count)]
    arity = [1 if op in (api.NOT, api.COPY) else 3 if op in (api.MUX, api.NMUX) else 2 for op in range(14)]
    try:
        for zero_copy in (1, 0):
            for o in outs:
                o.tlwehost[:] = pos.POISON
            with pos.options(api, dict(sched_zero_copy=zero_copy)):
                for g in range(count):
                    op = int(G.t_ops[g])
                    api.Apply(op, outs[g], *[cin[i][g] for i in range(arity[op])], sts[g % nst])
                api.Synchronize()
            got = np.stack([o.tlwehost for o in outs])
            pos.assert_every_row(got, G.want, f"per-gate API, 256 streams, sched_zero_copy {zero_copy}, {count} gates", _groupings(engine) + (nst, 2048))
    finally:
        api.Synchronize()
        for s in sts:
            s.Destroy()
        for lst in cin + [outs]:
            for c in lst:
                c.release()


# ---------------------------------------------------------------------------------------------------------------------------------
# d. the N = 2048 ring
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keys2(oracle, keys):
    return ol.KeysLvl2(oracle, keys, seed=7)


@pytest.fixture(scope="module")
def ring(engine, keys, keys2):
    engine.lvl2_initialize(keys2.bk, keys2.ksk)
    if "ring" not in _cache:
        _cache["ring"] = Gates(engine, keys, 0, ol.MU, lambda ops, a, b, c: keys2.gate_batch(ops, a, b, c), 9300, 4096)
    return _cache["ring"]


def _ring_launch(eng):
    return lambda ops, out, a, b, c, count: eng.lvl2_gate_batch(ops, out, a, b, c, count=count)


def _ring_counts(c):
    return [1, 7, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1]


def test_ring_automatic_rule(engine, ring):
    c = engine.api.device_cus()
    for count in _ring_counts(c) + [4096]:
        _check(engine, ring, count, "N = 2048 ring, automatic rule", launch=_ring_launch(engine))


@pytest.mark.parametrize("kernel", [0, 1])
def test_ring_forced_kernels(engine, ring, kernel):
    c = engine.api.device_cus()
    for count in (7, c + 1, 2 * c + 1):
        _check(engine, ring, count, f"N = 2048 ring, lvl2_kernel {kernel}", dict(lvl2_kernel=kernel), launch=_ring_launch(engine))


def test_ring_other_cu_count(engine, ring):
    for count in _ring_counts(40):
        _check(engine, ring, count, "N = 2048 ring, cus_override 40", dict(cus_override=40), launch=_ring_launch(engine))


def test_ring_through_lvl0_ring_option(engine, ring):
    for count in (17, 300):
        _check(engine, ring, count, "lvl0_ring 2048 through cufhe_amd_gate_batch", dict(lvl0_ring=2048), launch=_batch(engine, 0))


@pytest.mark.parametrize("opts", [{}, dict(ks_wg_threshold=0, ks_per_wg=16, ks_slices=64)], ids=["default", "16x64"])
def test_ring_keyswitch_alone_4096(engine, ring, keys2, opts):
    count = 4096
    rng = np.random.default_rng(9400)
    t2 = rng.integers(0, 2**64, size=(D, ol.LVL2_WORDS), dtype=np.uint64)
    t2[0] = 0
    t2[1] = np.uint64(2**64 - 1)
    t2[2, ol.N2] = np.uint64(0x7FFFFFFF80000000)             # rounding of b carries into bit 31
    t2[3, : ol.N2] = np.uint64(0x8000000000000000)           # every digit at its extreme
    want = np.stack(_pmap(lambda d: keys2.keyswitch(t2[d]), range(D)))
    d2 = _up(engine, pos.tile(t2, count))
    d0 = _up(engine, pos.poison(count * (ol.n + 1)))
    with pos.options(engine.api, opts):
        engine.lvl2_keyswitch_batch(d2, d0, count)
        got = d0.download().reshape(count, ol.n + 1)
    pos.assert_every_row(got, want, f"lvl20 key switch alone, {opts}, {count} ciphertexts", _groupings(engine))


# ---------------------------------------------------------------------------------------------------------------------------------
# e. the other parameter sets
# ---------------------------------------------------------------------------------------------------------------------------------
PS_FACTOR = {"smallmod": 4, "k2n512": 5, "cggi16": 6}       # plan::ps_batch_from = factor x CUs + 1 rotations (include/cufhe_amd.h: 1025 / 1281 / 1537)


@pytest.fixture(scope="module", params=list(PS_FACTOR))
def pset(request, engine):
    name = request.param
    L = ol.load_set(name)
    K = ol.Keys(L, seed=5)
    idx = engine.api.ps_index(name)
    engine.api.ps_initialize(idx, K.bk, K.ksk)
    return name, idx, L, K


def _psgates(engine, pset, level):
    name, idx, L, K = pset
    if (name, level) not in _cache:
        mu = engine.api.ps_params(idx).mu
        _cache[name, level] = Gates(engine, K, level, mu, lambda ops, a, b, c: K.gate_batch(ops, level, a, b, c), 9500 + 10 * level, 4096)
    return _cache[name, level]


@pytest.fixture(scope="module", params=[0, 1])
def psgates(request, engine, pset):
    return _psgates(engine, pset, request.param)


def _ps_launch(eng, idx, level):
    return lambda ops, out, a, b, c, count: eng.api.ps_gate_batch(idx, ops, out, a, b, c, count=count, level=level)


@pytest.mark.parametrize("threshold", [1, 1 << 30], ids=["wave-per-rotation", "workgroup-per-rotation"])
def test_paramset_forced_shapes(engine, pset, psgates, threshold):
    name, idx, L, K = pset
    for count in (1, 7, 8, 9, 12, 13, 25, 300):
        _check(engine, psgates, count, f"{name}, ps_batch_threshold {threshold}", dict(ps_batch_threshold=threshold), launch=_ps_launch(engine, idx, psgates.level))


@pytest.mark.parametrize("cus", [0, 40], ids=["device", "cus40"])
def test_paramset_automatic_rule(engine, pset, psgates, cus):
    """T - 1, T, T + 1 gates of the tiled set (14 rotations per 14 gates, so the launch sits on the rule's boundary) and, because MUX
    and NOT make the rotation count differ from the gate count, exactly T - 1, T, T + 1 rotations through ps_blind_rotate_batch"""
    name, idx, L, K = pset
    api = engine.api
    with pos.options(api, dict(cus_override=cus)):
        c = api.device_cus()
    T = PS_FACTOR[name] * c + 1
    if c == 256:
        assert T == {"smallmod": 1025, "k2n512": 1281, "cggi16": 1537}[name]
    for count in (T - 1, T, T + 1):
        _check(engine, psgates, count, f"{name}, automatic rule at {c} CUs (T = {T})", dict(cus_override=cus), launch=_ps_launch(engine, idx, psgates.level))
    if psgates.level == 0:
        rng = np.random.default_rng(9600)
        tl = _corner_tlwe0(rng, K.n, D)
        want = np.stack(_pmap(lambda d: K.blind_rotate(tl[d], 3), range(D)))
        dt = _up(engine, pos.tile(tl, T + 1))
        for count in (T - 1, T, T + 1):
            dacc = _up(engine, pos.poison(count * want.shape[1]))
            with pos.options(api, dict(cus_override=cus)):
                api.ps_blind_rotate_batch(idx, dt, dacc, count, 3)
                got = dacc.download().reshape(count, -1)
            pos.assert_every_row(got, want, f"{name}, {count} rotations of 3 steps at {c} CUs (T = {T})", _groupings(engine))


def test_paramset_4096(engine, pset):
    name, idx, L, K = pset
    _check(engine, _psgates(engine, pset, 0), 4096, f"{name}", launch=_ps_launch(engine, idx, 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# f. TRLWE-level batches of the default path and of every set
# ---------------------------------------------------------------------------------------------------------------------------------
TRLWE_COUNTS = (1, 3, 4, 5, 9, 300, 1031)


def _trlwe_path(name, engine, keys):
    """(name, K, l, calls): the entry points of one path behind common names"""
    api = engine.api
    if name == "default":
        calls = dict(rotate=lambda t, a, c, s: api.blind_rotate_batch(t, a, c, s),
                     bootstrap=lambda o, i, c: api.bootstrap_batch(o, i, c),                    # lvl0 -> lvl0 (rotate, extract, key switch)
                     refresh=lambda o, i, c: api.refresh_batch(i, o, c),
                     seiks=lambda o, i, c: api.sample_extract_keyswitch_batch(i, o, c),
                     to_ntt=lambda g, n_, c: api.trgsw_to_ntt_batch(g, n_, c),
                     cmux=lambda n_, c1, c0, r, c: api.cmux_batch(n_, c1, c0, r, c), limbs=1)
        return name, keys, 3, calls
    L = ol.load_set(name)
    K = ol.Keys(L, seed=5)
    idx = api.ps_index(name)
    api.ps_initialize(idx, K.bk, K.ksk)
    calls = dict(rotate=lambda t, a, c, s: api.ps_blind_rotate_batch(idx, t, a, c, s),
                 bootstrap=lambda o, i, c: api.ps_trlwe_op_batch(idx, api.TL_BOOTSTRAP, o, i, c),   # lvl0 -> TRLWE
                 refresh=lambda o, i, c: api.ps_trlwe_op_batch(idx, api.TL_REFRESH, o, i, c),
                 seiks=lambda o, i, c: api.ps_trlwe_op_batch(idx, api.TL_SEIKS, o, i, c),
                 to_ntt=lambda g, n_, c: api.ps_trgsw_to_ntt_batch(idx, g, n_, c),
                 cmux=lambda n_, c1, c0, r, c: api.ps_cmux_batch(idx, n_, c1, c0, r, c), limbs=api.ps_params(idx).key_limbs)
    return name, K, ol.set_params(L)[1]["l"], calls


@pytest.fixture(scope="module", params=["default"] + list(PS_FACTOR))
def trlwe_path(request, engine, keys):
    return _trlwe_path(request.param, engine, keys)


@pytest.fixture(scope="module", params=["default", "k2n512", "cggi16"])
def cmux_path(request, engine, keys):
    """the paths that have TRGSW2NTT / CMUXNTT: not the small-modulus set (as the reference's build, src/cufhe_gates_gpu.cu:68-86)"""
    return _trlwe_path(request.param, engine, keys)


@pytest.fixture(scope="module")
def trlwe_ref(trlwe_path):
    """the D distinct inputs and expected words of every TRLWE-level operation of the path"""
    name, K, l, calls = trlwe_path
    rng = np.random.default_rng(9700)
    t0 = time.time()
    tl = _corner_tlwe0(rng, K.n, D)

    def extract(acc):
        t = np.zeros(K.words[1], np.uint32)
        K.L.orc_sample_extract0(t, np.ascontiguousarray(acc))
        return t
    r = dict(tl=tl)
    r["acc3"] = np.stack(_pmap(lambda d: K.blind_rotate(tl[d], 3), range(D)))
    r["acc"] = np.stack(_pmap(lambda d: K.blind_rotate(tl[d], -1), range(D)))
    r["seiks"] = np.stack(_pmap(lambda d: K.keyswitch(extract(r["acc"][d])), range(D)))      # of the TRLWEs r["acc"]
    r["refresh"] = np.stack(_pmap(lambda d: K.blind_rotate(r["seiks"][d], -1), range(D)))
    print(f"\n[positions] reference of {D} distinct TRLWE-level cases, {name}: {time.time() - t0:.2f} s")
    return r


def _rows(eng, run, din, count, want, label):
    dout = _up(eng, pos.poison(count * want[0].size, want.dtype))
    run(dout, din, count)
    got = dout.download()
    if want.dtype == np.uint64:
        got = got.view(np.uint64)
    pos.assert_every_row(got.reshape((count,) + want.shape[1:]), want, f"{label}, {count} rows", _groupings(eng))


@pytest.mark.parametrize("count", TRLWE_COUNTS)
def test_trlwe_level_batches(engine, trlwe_path, trlwe_ref, count):
    name, K, l, calls = trlwe_path
    r = trlwe_ref
    dtl = _up(engine, pos.tile(r["tl"], count))
    dacc = _up(engine, pos.tile(r["acc"], count))
    _rows(engine, lambda o, i, c: calls["rotate"](i, o, c, 3), dtl, count, r["acc3"], f"{name}: blind_rotate_batch, 3 steps")
    _rows(engine, lambda o, i, c: calls["rotate"](i, o, c, -1), dtl, count, r["acc"], f"{name}: blind_rotate_batch, all steps")
    _rows(engine, calls["bootstrap"], dtl, count, r["seiks"] if name == "default" else r["acc"], f"{name}: bootstrap_batch")
    _rows(engine, calls["refresh"], dacc, count, r["refresh"], f"{name}: refresh_batch")
    _rows(engine, calls["seiks"], dacc, count, r["seiks"], f"{name}: sample_extract_keyswitch_batch")


@pytest.fixture(scope="module")
def cmux_ref(cmux_path):
    name, K, l, calls = cmux_path
    rng = np.random.default_rng(9800)
    trlwe_words, trgsw_words = (K.k + 1) * K.N, (K.k + 1) * l * (K.k + 1) * K.N
    tg = U32(rng, (D, trgsw_words))
    ext = np.array((0x80000000, 0x7FFFFFFF, 0, 0xFFFFFFFF, 0x80000001), np.uint32)
    tg[1] = ext[rng.integers(0, ext.size, trgsw_words)]
    tg[2] = 0x80000000
    tg[3] = np.asarray(K.bk, np.uint32).reshape(K.n, trgsw_words)[5]        # a real TRGSW encryption of a key bit
    c1, c0 = U32(rng, (D, trlwe_words)), U32(rng, (D, trlwe_words))
    c1[4] = c0[4]                                                           # zero difference: res = c0
    c1[5] = c0[5] + np.uint32(0x7FFFFFFF)

    def one(d):
        w = np.zeros(trlwe_words, np.uint32)
        K.L.orc_cmux(w, np.ascontiguousarray(tg[d]), np.ascontiguousarray(c1[d]), np.ascontiguousarray(c0[d]))
        return w
    return tg, c1, c0, np.stack(_pmap(one, range(D)))


@pytest.mark.parametrize("count", TRLWE_COUNTS)
def test_trgsw_to_ntt_and_cmux_batches(engine, cmux_path, cmux_ref, count):
    """TRGSW2NTT + CMUXNTT put four waves in a workgroup: every row of the product, also in place on c0 and on c1"""
    name, K, l, calls = cmux_path
    tg, c1, c0, want = cmux_ref
    api = engine.api
    dntt = _up(engine, pos.poison(count * tg.shape[1] * 2 * calls["limbs"]))
    calls["to_ntt"](_up(engine, pos.tile(tg, count)), dntt, count)
    d1, d0 = _up(engine, pos.tile(c1, count)), _up(engine, pos.tile(c0, count))
    dres = _up(engine, pos.poison(count * want.shape[1]))
    calls["cmux"](dntt, d1, d0, dres, count)
    pos.assert_every_row(dres.download().reshape(count, -1), want, f"{name}: CMUXNTT of TRGSW2NTT, {count} rows", _groupings(engine))
    assert np.array_equal(d1.download().reshape(count, -1), pos.tile(c1, count)) and np.array_equal(d0.download().reshape(count, -1), pos.tile(c0, count))
    calls["cmux"](dntt, d1, d0, d0, count)
    pos.assert_every_row(d0.download().reshape(count, -1), want, f"{name}: CMUXNTT in place on c0, {count} rows", _groupings(engine))
    d0 = _up(engine, pos.tile(c0, count))
    calls["cmux"](dntt, d1, d0, d1, count)
    pos.assert_every_row(d1.download().reshape(count, -1), want, f"{name}: CMUXNTT in place on c1, {count} rows", _groupings(engine))
    api.Synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# g. user gates and multi-output gates in one cufhe_amd_gate_list
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def user_defs(engine, keys):
    """three multi-output definitions (8 / 4 / 2 outputs, arities 3 / 2 / 1) and two single user gates, with random test vectors
    and offsets; dropped again (CleanUp) when the module ends"""
    import multi_output_checker as mc      # noqa: F401  (importable: the references below)
    rng = np.random.default_rng(9900)
    defs = []
    for nout, c in ((8, (1, -2, 1)), (4, (2, 1, 0)), (2, (-3, 0, 0)), (1, (1, 1, 0)), (1, (-1, 2, -1))):
        tv, off = U32(rng, ol.N), int(rng.integers(0, 1 << 32))
        defs.append(dict(c=c, off=off, tv=tv, nout=nout, op=engine.define_gate(c, off, tv, nout=nout)))
    yield defs
    engine.CleanUp()
    engine.SetGPUNum(1)
    engine.Initialize(keys.bk, keys.ksk)


@pytest.fixture(scope="module", params=[0, 1])
def user_list(request, engine, keys, user_defs):
    """The period of DC = 23 outputs: 8 + 4 + 2 sibling outputs of three evaluations, two single user gates and seven built-in ops, in
    a fixed shuffled order (siblings are not neighbours); evaluation e of period q reads row 12 q + e of every operand, so no two
    periods share an evaluation.  (ops [DC], evaluation of each output [DC], inputs [12][words] x 3, expected words [DC][words])"""
    import multi_output_checker as mc
    import user_gate_checker as uc
    level, api = request.param, engine.api
    assert DC == 23
    rng = np.random.default_rng(9910 + level)
    words = ol.LVL_WORDS[level]
    ins = [U32(rng, (12, words)) for _ in range(3)]
    builtin = [api.NAND, api.MUX, api.NOT, api.XOR, api.COPY, api.NMUX, api.AND]
    t0 = time.time()

    def evaluate(e):
        row = [a[e] for a in ins]
        if e < 3:
            d = user_defs[e]
            return mc.multi_gate_one(keys, level, d["c"], d["off"], d["tv"], d["nout"], row)
        if e < 5:
            d = user_defs[e]
            return [uc.user_gate_one(keys, level, d["c"], d["off"], d["tv"], row)]
        return [keys.gate_batch(builtin[e - 5], level, row[0][None], row[1][None], row[2][None])[0]]
    res = _pmap(evaluate, range(12))
    print(f"\n[positions] checkers of 3 multi-output + 2 single user gates + 7 built-in ops, level {level}: {time.time() - t0:.2f} s")
    outputs = []                                             # (op, evaluation, expected words)
    for e in range(12):
        for j, w in enumerate(res[e]):
            op = api.user_op_output(user_defs[e]["op"], j) if e < 3 else user_defs[e]["op"] if e < 5 else builtin[e - 5]
            outputs.append((op, e, w))
    assert len(outputs) == DC
    outputs = [outputs[i] for i in np.random.default_rng(5).permutation(DC)]
    return level, np.array([o[0] for o in outputs], np.int32), np.array([o[1] for o in outputs]), ins, np.stack([o[2] for o in outputs])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_user_and_multi_output_gates_in_one_list(engine, user_list, shape):
    level, ops, evals, ins, want = user_list
    api = engine.api
    words = ol.LVL_WORDS[level]
    for count in (300, 2100):
        periods = (count + DC - 1) // DC
        dins = [_up(engine, np.tile(a, (periods, 1))) for a in ins]
        dout = _up(engine, pos.poison(count * words))
        g = np.arange(count)
        rows = (g // DC) * 12 + evals[g % DC]
        t_ops = pos.tile(ops, count)
        arr = lambda base, r, stride: (ctypes.c_void_p * count)(*(base + r.astype(np.int64) * stride).tolist())  # noqa: E731
        with pos.options(api, SHAPES[shape]):
            engine.check(engine.lib.cufhe_amd_gate_list(0, None, level, count, t_ops.ctypes.data, arr(dout.ptr, g, words * 4),
                                                        arr(dins[0].ptr, rows, words * 4), arr(dins[1].ptr, rows, words * 4),
                                                        arr(dins[2].ptr, rows, words * 4)))
            engine.Synchronize()
            got = dout.download().reshape(count, words)
        pos.assert_every_row(got, want, f"user / multi-output / built-in gates in one list, shape {shape}, level {level}, {count} outputs", _groupings(engine))


# ---------------------------------------------------------------------------------------------------------------------------------
# h. circuit bootstrapping
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cb_case(engine, keys, keys2, ring):
    """a private key-switching key of random words (word checks need no encryption), DC distinct inputs with the corner cases, and the
    checker's stage 1 and TRGSW words for them"""
    import cb_checker as cb
    key = np.random.default_rng(2024).integers(0, 2**32, size=cb.PKS_KEY_WORDS, dtype=np.uint32)
    engine.api.cb_initialize(key)
    tl = _corner_tlwe0(np.random.default_rng(9950), ol.n, DC)
    t0 = time.time()
    cb.cb_rotate_one(keys2, tl[0])                           # alone first: the oracle builds its tables once
    t1 = time.time()
    stage1 = cb.cb_rotate_batch(keys2, tl, threads=THREADS)
    t2 = time.time()
    trgsw = cb.trgsw_from_stage1(key, stage1)
    print(f"\n[positions] cb_checker: one circuit bootstrap's stage 1 alone {t1 - t0:.2f} s, {DC} on {THREADS} threads {t2 - t1:.2f} s, "
          f"their private key switches {time.time() - t2:.2f} s")
    return cb, tl, stage1, trgsw


@pytest.mark.parametrize("count,kernel", [(90, -1), (90, 0), (90, 1), (700, -1)])
def test_cb_rotate_batch(engine, cb_case, count, kernel):
    cb, tl, stage1, trgsw = cb_case
    d0 = _up(engine, pos.tile(tl, count))
    d2 = _up(engine, pos.poison(count * cb.CB_L * cb.PKS_IN, np.uint64))
    with pos.options(engine.api, dict(lvl2_kernel=kernel)):
        engine.api.cb_rotate_batch(d0, d2, count)
        got = d2.download().view(np.uint64).reshape(count, cb.CB_L, cb.PKS_IN)
    pos.assert_every_row(got, stage1, f"cb_rotate_batch, lvl2_kernel {kernel}, {count} inputs ({3 * count} rotations)", _groupings(engine))


def test_circuit_bootstrap_batch(engine, cb_case):
    cb, tl, stage1, trgsw = cb_case
    api, count = engine.api, 90
    d0 = _up(engine, pos.tile(tl, count))
    dt = _up(engine, pos.poison(count * cb.TRGSW_WORDS))
    dn = _up(engine, pos.poison(count * cb.TRGSW_WORDS * 2))
    api.circuit_bootstrap_batch(d0, count, trgsw=dt, trgsw_ntt=dn)
    torus = dt.download().reshape(count, 2 * cb.CB_L, 2, ol.N)
    pos.assert_every_row(torus, trgsw, f"circuit_bootstrap_batch torus words, {count} inputs", _groupings(engine))
    dn2 = _up(engine, pos.poison(count * cb.TRGSW_WORDS * 2))
    api.trgsw_to_ntt_batch(dt, dn2, count)
    ntt, ntt2 = dn.download().reshape(count, -1), dn2.download().reshape(count, -1)
    assert np.array_equal(ntt, ntt2), "NTT-domain output != trgsw_to_ntt_batch of the torus output"      # bit for bit, all rows
    pos.assert_every_row(ntt, np.ascontiguousarray(ntt2[:DC]), f"circuit_bootstrap_batch NTT words, {count} inputs", _groupings(engine))
