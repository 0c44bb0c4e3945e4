"""Every batched entry point writes its documented outputs and nothing else (tests/footprint.py).

For every case of footprint.CASES, every option set and every count (0, 1 and U + 1, U the items one workgroup or tile takes) all
device operands of the call lie in ONE allocation between guards.  After the call on the null stream the whole allocation is
downloaded once and, in this order: the status is 0; every row of every output equals the reference the suite already trusts (exact,
all rows); no other word of the allocation changed -- no guard word, no pad word, no word of an input.  The aliasings the header
permits run once at U + 1 with the shared operand declared inout; the ones it forbids must return -1 and change nothing; count 0
must change nothing (cufhe_amd_pack_batch: its documented zeroing).  Three launches of one row too many, inside owned memory, show
that the harness sees a real kernel write row `count`.

References are computed once per module for the 7 distinct inputs (positions.PRIMES[0]) a batch is tiled from; the N = 2048 ring runs a
workgroup per rotation, so its counts stop at 3 and its Python checkers run for the three inputs that reach the device.
"""
import ctypes
import time

import numpy as np
import pytest

import cb_checker as cb
import footprint as fp
import lut_checker as lc
import lvl2_user_gate_checker as lc2
import multi_output_checker as mc
import oracle_lib as ol
import pack_checker as pk
import packed_rom_checker as pr
import positions as pos
import user_gate_checker as uc
from test_gpu_circuit_bootstrap import random_words  # noqa: F401  (fixture: the private key-switching key of random words)
from test_gpu_positions import SHAPES, _corner_tlwe0, _pmap, keys2  # noqa: F401  (keys2: fixture, the lvl02 / lvl20 keys)

pytestmark = pytest.mark.gpu

D = pos.PRIMES[0]
N, n, N2 = ol.N, ol.n, ol.N2
W0, W1, W2 = n + 1, N + 1, N2 + 1
TRLWE, TRGSW = 2 * N, 12 * N
U32, I32, U64, F64 = np.uint32, np.int32, np.uint64, np.float64
O = fp.Operand
SRC7 = np.array([0, 1, 2, 2, 4, 5, 6], I32)                    # source 2 named twice, source 3 by nobody
IDX7 = np.array([0, N - 1, 1, 63, 64, 511, 1022], I32)
EXPS7 = np.array([0, 1, N - 1, N, 2 * N - 1, 777, 1500], I32)
RING_ROWS = 3        # the N = 2048 ring runs a workgroup per rotation: counts 0, 1 and 3 use the first three distinct inputs only
NAND, MUX, NOT, COPY, XOR, NMUX, AND = (ol.OPS.index(k) for k in ("NAND", "MUX", "NOT", "COPY", "XOR", "NMUX", "AND"))


def rnd(seed, shape, dtype=U32):
    bits = 64 if np.dtype(dtype) == U64 else 32
    return np.random.default_rng(seed).integers(0, 2 ** bits, size=shape, dtype=U64).astype(dtype)


def tiled(distinct, count):
    return pos.tile(distinct, count)


class DeviceBackend:
    """the arena in one device allocation of the library's own allocator (cufhe_amd_malloc)"""

    def __init__(self, api):
        self.api = api

    def alloc(self, words):
        self.buf = self.api.DeviceBuffer(words)
        return self.buf.ptr

    def upload(self, host):
        self.buf.upload(host)

    def download(self):
        return self.buf.download()


class Call:
    """operands, the words of the inputs, fn(arena) -> status, and the expected rows of every output:
    want[name] = ("tiled", distinct) | ("full", rows) | ("at", slots, rows) | ("first", rows: output row g equals rows[g])"""

    def __init__(self, operands, fills, fn, want, written=None):
        self.operands, self.fills, self.fn, self.want, self.written = operands, fills, fn, want, written or {}


# ---------------------------------------------------------------------------------------------------------------------------------
# the module's device state and references
# ---------------------------------------------------------------------------------------------------------------------------------
class Env:
    def __init__(self, engine, oracle, keys, keys2, cb_key):
        self.engine, self.api, self.lib, self.oracle, self.keys, self.keys2, self.cb_key = engine, engine.api, engine.lib, oracle, keys, keys2, cb_key
        self._cache = {}
        api = self.api
        engine.CleanUp()
        engine.SetGPUNum(1)
        engine.Initialize(keys.bk, keys.ksk)
        engine.lvl2_initialize(keys2.bk, keys2.ksk)
        api.cb_initialize(cb_key)
        self.pack_key = rnd(900, pk.KEY_WORDS)
        api.pack_initialize(self.pack_key)
        # user gates of the default ring: one single-output gate with a test vector, a 2-output and an 8-output definition
        self.udefs = {}
        for name, nout, c in (("single", 1, (1, 1, 0)), ("two", 2, (2, 1, 0)), ("eight", 8, (1, -2, 1))):
            tv, off = rnd(9900 + nout, N), int(rnd(9910 + nout, 1)[0])
            self.udefs[name] = dict(c=c, off=off, tv=tv, nout=nout, op=engine.define_gate(c, off, tv, nout=nout))
        # user gates of the N = 2048 ring: arity 1 with a test vector, arity 2 without, arity 3 with one, and a p = 8 table
        tv0, tv2 = rnd(1, N2, U64), rnd(2, N2, U64)
        tv0[[0, 5, N2 - 1]] = [0, 1 << 63, 2 ** 64 - 1]
        values = (np.random.default_rng(77).permutation(8).astype(U64) << U64(60)) + U64(12345)
        self.spec2 = {"one": ((1, 0, 0), 0, tv0), "two": ((3, -2, 0), 0x12345678, None), "three": ((1, -1, 2), 0xF0000001, tv2),
                      "table": ((1, 0, 0), 0, lc2.test_vector(values))}
        self.op2 = {k: engine.lvl2_define_gate(*s) for k, s in self.spec2.items()}
        self.sets = {}

    def close(self):
        """drop the user gates, the packing key and the circuit-bootstrap key: the modules that follow start from Initialize"""
        self.engine.CleanUp()
        self.engine.SetGPUNum(1)
        self.engine.Initialize(self.keys.bk, self.keys.ksk)

    def once(self, key, make):
        if key not in self._cache:
            t0 = time.time()
            self._cache[key] = make()
            if time.time() - t0 > 0.5:
                print(f"\n[footprint] reference {key}: {time.time() - t0:.2f} s")
        return self._cache[key]

    def device_rows(self, fn, rows, row_words):
        """rows computed on the device into an exact-size buffer, as the existing tests do (a reference that is itself GPU output:
        the NTT-domain words, which are opaque to callers and tied to the oracle through CMUXNTT)"""
        d = self.api.DeviceBuffer(rows * row_words)
        fn(d)
        self.engine.Synchronize()
        out = d.download().reshape(rows, row_words)
        d.free()
        return out

    # ---- default path ----
    @property
    def tl7(self):
        return self.once("tl7", lambda: _corner_tlwe0(np.random.default_rng(9700), n, D))

    def acc(self, steps):
        return self.once(("acc", steps), lambda: np.stack(_pmap(lambda d: self.keys.blind_rotate(self.tl7[d], steps), range(D))))

    def _extract0(self, K, acc):
        t = np.zeros(K.words[1], U32)
        K.L.orc_sample_extract0(t, np.ascontiguousarray(acc))
        return t

    @property
    def seiks(self):
        return self.once("seiks", lambda: np.stack(_pmap(lambda d: self.keys.keyswitch(self._extract0(self.keys, self.acc(-1)[d])), range(D))))

    @property
    def refresh(self):
        return self.once("refresh", lambda: np.stack(_pmap(lambda d: self.keys.blind_rotate(self.seiks[d], -1), range(D))))

    @property
    def t1(self):
        def make():
            t = rnd(4100, (D, W1))
            t[0] = 0
            t[1] = 0xFFFFFFFF
            t[2, :N] = 0xFFFFFFFF
            return t
        return self.once("t1", make)

    @property
    def ks(self):
        return self.once("ks", lambda: np.stack(_pmap(lambda d: self.keys.keyswitch(self.t1[d]), range(D))))

    @property
    def trl(self):
        return self.once("trl", lambda: rnd(600, (D, TRLWE)))

    def extract(self, shared):
        return self.once(("extract", shared), lambda: np.stack([pr.extract_formula(self.trl[SRC7[d] if shared else d], int(IDX7[d])) for d in range(D)]))

    def extract_ks(self, shared):
        return self.once(("extract_ks", shared), lambda: np.stack(_pmap(lambda d: self.keys.keyswitch(self.extract(shared)[d]), range(D))))

    def cmux_data(self, K):
        """the corner TRGSWs and TRLWEs of test_gpu_positions.py::cmux_ref, D of them, and the oracle's CMUXNTT"""
        def make():
            l = ol.set_params(K.L)[1]["l"]
            tw, gw = (K.k + 1) * K.N, (K.k + 1) * l * (K.k + 1) * K.N
            rng = np.random.default_rng(9800)
            tg = rnd(9801, (D, gw))
            ext = np.array((0x80000000, 0x7FFFFFFF, 0, 0xFFFFFFFF, 0x80000001), U32)
            tg[1] = ext[rng.integers(0, ext.size, gw)]
            tg[2] = 0x80000000
            tg[3] = np.asarray(K.bk, U32).reshape(K.n, gw)[5]
            c1, c0 = rnd(9802, (D, tw)), rnd(9803, (D, tw))
            c1[4] = c0[4]
            c1[5] = c0[5] + U32(0x7FFFFFFF)

            def one(d):
                w = np.zeros(tw, U32)
                K.L.orc_cmux(w, np.ascontiguousarray(tg[d]), np.ascontiguousarray(c1[d]), np.ascontiguousarray(c0[d]))
                return w
            return tg, c1, c0, np.stack(_pmap(one, range(D)))
        return self.once(("cmux", K.set_name), make)

    def ntt_of(self, key, trgsw_rows, ps=None, limbs=1):
        """the NTT-domain doubles of torus-domain TRGSW rows"""
        def make():
            rows, gw = trgsw_rows.shape
            src = self.api.DeviceBuffer(rows * gw).upload(trgsw_rows)
            if ps is None:
                out = self.device_rows(lambda d: self.api.trgsw_to_ntt_batch(src, d, rows), rows, gw * 2 * limbs)
            else:
                out = self.device_rows(lambda d: self.api.ps_trgsw_to_ntt_batch(ps, src, d, rows), rows, gw * 2 * limbs)
            src.free()
            return np.ascontiguousarray(out).view(F64).reshape(rows, gw * limbs)
        return self.once(("ntt", key), make)

    @property
    def selector(self):
        return self.once("selector", lambda: pr.selector(self.keys, 1))

    @property
    def cmux_rotate(self):
        return self.once("cmux_rotate", lambda: np.stack(_pmap(lambda d: pr.cmux_rotate(self.oracle, self.selector, self.trl[d], int(EXPS7[d])), range(D))))

    @property
    def rotate(self):
        return self.once("rotate", lambda: np.stack([pr.rotate(self.trl[d], int(EXPS7[d])) for d in range(D)]))

    def spread(self, stride, reps):
        return self.once(("spread", stride, reps), lambda: np.stack(_pmap(lambda d: lc.spread(self.trl[d], stride, reps), range(D))))

    @property
    def poly(self):
        def make():
            rng = np.random.default_rng(7)
            a = rng.integers(-32, 32, size=(D, N), dtype=I32)
            a[0], a[1] = 31, -32
            a[2] = rng.integers(-128, 129, size=N)
            b = rnd(8, (D, N))
            b[0], b[1], b[3] = 0xFFFFFFFF, 0x80000000, 0
            want = np.zeros((D, N), U32)
            for d in range(D):
                self.oracle.orc_polymul_schoolbook(want[d], np.ascontiguousarray(a[d]), np.ascontiguousarray(b[d]))
            return a, b, want
        return self.once("poly", make)

    @property
    def poly512(self):
        def make():
            rng = np.random.default_rng(8)
            m = 512
            a = rng.integers(-128, 129, size=(D, m), dtype=I32)
            a[0], a[1] = 128, -128
            b = rnd(9, (D, m))
            b[0], b[1], b[2] = 0x80000000, 0x7FFFFFFF, 0
            want = np.zeros((D, m), U32)
            for d in range(D):
                full = np.convolve(a[d].astype(np.int64), b[d].astype(I32).astype(np.int64))
                full = np.concatenate([full, np.zeros(2 * m - full.size, np.int64)])
                want[d] = ((full[:m] - full[m:]) & 0xFFFFFFFF).astype(U32)
            return a, b, want
        return self.once("poly512", make)

    @property
    def lut_x(self):
        def make():
            x = rnd(1600, (D, W0))
            x[0, n] = 0                   # bbar = 2N: the unrotated table
            x[1, n] = 0xFFFFFFFF          # bbar = 1 at nout = 1
            x[2, :4] = 0
            return x
        return self.once("lut_x", make)

    @property
    def tables(self):
        def make():
            t = rnd(1601, (D, TRLWE))
            t[5, :N] = 0                  # A = 0: the plain-gate case of the first TRGSW row
            return t
        return self.once("tables", make)

    def lut_rotate(self, nout):
        s = mc.shift_of(nout)
        return self.once(("lut_rotate", nout), lambda: np.stack(_pmap(lambda d: lc.lut_rotate(self.keys, self.lut_x[d], self.tables[SRC7[d]], s, 3), range(D))))

    def lut_lookup(self, nout):
        return self.once(("lut_lookup", nout), lambda: np.stack(_pmap(
            lambda d: lc.lut_lookup(self.keys, self.lut_x[d], self.tables[SRC7[d]], nout).reshape(nout * W0), range(D))))

    # ---- gates of the default path: 15 ops over 7 evaluations (the outputs of one definition share their operands, so one rotation)
    def gate_list(self, level):
        def make():
            K, u = self.keys, self.udefs
            bits = np.random.default_rng(9100 + level).integers(0, 2, size=(3, D)).astype(np.uint8)
            ins = [K.encrypt(bits[i], level, seed=9101 + 10 * level + i) for i in range(3)]
            ins[0][0, :4] = 0
            ins[1][0, :4] = 0                                    # a run of zero words enters the rotation (level 0) / the key switch
            ins[0][6, :] = 0x7FFFFFFF
            ins[1][6, :] = 0x7FFFFFFF
            ops, evals = [NAND, MUX, NOT, COPY, u["single"]["op"]], [0, 1, 2, 3, 4]
            for e, name in ((5, "two"), (6, "eight")):
                for j in range(u[name]["nout"]):
                    ops.append(self.api.user_op_output(u[name]["op"], j))
                    evals.append(e)

            def evaluate(e):
                row = [a[e] for a in ins]
                if e < 4:
                    return [K.gate_batch(ops[e], level, row[0][None], row[1][None], row[2][None])[0]]
                d = u[("single", "two", "eight")[e - 4]]
                if d["nout"] == 1:
                    return [uc.user_gate_one(K, level, d["c"], d["off"], d["tv"], row)]
                return mc.multi_gate_one(K, level, d["c"], d["off"], d["tv"], d["nout"], row)
            res = _pmap(evaluate, range(D))
            want = np.stack([w for e in range(D) for w in res[e]])
            assert len(ops) == 15 == want.shape[0]
            return np.array(ops, I32), np.array(evals), ins, want
        return self.once(("gate_list", level), make)

    def gates(self, level, count):
        """ops, the rows of the three operands and the expected rows of `count` gates: gate g is entry g % 15 of the list"""
        ops, evals, ins, want = self.gate_list(level)
        g = np.arange(count)
        return ops[g % 15].astype(I32), [np.ascontiguousarray(a[evals[g % 15]]) for a in ins], np.ascontiguousarray(want[g % 15])

    # ---- N = 2048 ring ----
    @property
    def ring_gates(self):
        def make():
            K2 = self.keys2
            # the first three, which every run with rows reaches: a built-in op, the p = 8 table, the three-operand gate with a table
            names = [None, "table", "three", None, "one", "two", None]
            ops = np.array([NAND, self.op2["table"], self.op2["three"], MUX, self.op2["one"], self.op2["two"], NOT], I32)
            ins = [rnd(540 + i, (D, W0)) for i in range(3)]
            ins[0][0, n] = 0

            def one(d):
                if names[d] is None:
                    return K2.gate_batch(int(ops[d]), ins[0][d][None], ins[1][d][None], ins[2][d][None])[0]
                return lc2.user_gate_one(K2, *self.spec2[names[d]], [a[d] for a in ins])
            return ops, ins, np.stack(_pmap(one, range(RING_ROWS)))
        return self.once("ring_gates", make)

    def acc2(self, steps):
        return self.once(("acc2", steps), lambda: np.stack(_pmap(lambda d: self.keys2.blind_rotate(self.tl7[d], steps), range(D))))

    @property
    def user_rotate2(self):
        c, off, tv = self.spec2["one"]
        return self.once("user_rotate2", lambda: np.stack(_pmap(lambda d: lc2.user_rotate_one(self.keys2, c, off, tv, [self.tl7[d]], 2), range(D))))

    @property
    def user_extract2(self):
        ins = [rnd(540 + i, (D, W0)) for i in range(3)]          # the operands of ring_gates, but for input 0's b = 0
        ins[0][0, n] = 0
        return self.once("user_extract2", lambda: np.stack(lc2.on_threads(
            lambda d: lc2.user_extract_one(self.keys2, *self.spec2["three"], [a[d] for a in ins]), RING_ROWS)))

    @property
    def t2(self):
        def make():
            t = rnd(9400, (D, W2), U64)
            t[0] = 0
            t[1] = U64(2 ** 64 - 1)
            t[2, N2] = U64(0x7FFFFFFF80000000)
            t[3, :N2] = U64(0x8000000000000000)
            return t
        return self.once("t2", make)

    @property
    def ks2(self):
        return self.once("ks2", lambda: np.stack(_pmap(lambda d: self.keys2.keyswitch(self.t2[d]), range(D))))

    # ---- circuit bootstrapping, packing ----
    @property
    def stage1(self):
        """cb_checker.cb_rotate_one of the first three inputs, its l rotations per input on threads as well"""
        def one(i):
            d, r = divmod(i, cb.CB_L)
            row = cb.sample_extract0(self.keys2, cb.blind_rotate_mu(self.keys2, self.tl7[d], cb.cb_mu(r)))
            row[N2] += U64(cb.cb_mu(r))
            return row
        return self.once("stage1", lambda: np.stack(lc2.on_threads(one, RING_ROWS * cb.CB_L)).reshape(RING_ROWS, cb.CB_L, W2))

    @property
    def cb_trgsw(self):
        return self.once("cb_trgsw", lambda: cb.trgsw_from_stage1(self.cb_key, self.stage1).reshape(RING_ROWS, TRGSW))

    @property
    def pks_in(self):
        def make():
            b = rnd(24, (D, W2), U64)
            b[0] = 0
            b[1] = U64(2 ** 64 - 1)
            b[2, :] = U64(1 << 33) - U64(1)
            return b
        return self.once("pks_in", make)

    @property
    def pks(self):
        return self.once("pks", lambda: cb.private_keyswitch_batch(self.cb_key, self.pks_in).reshape(D, 2 * TRLWE))

    @property
    def pack_rows(self):
        def make():
            x = pk.edge_inputs(np.random.default_rng(1000), D)
            return x, np.stack([pk.pack_ks(self.pack_key, x[d]) for d in range(D)])
        return self.once("pack_rows", make)

    # ---- parameter sets ----
    def pset(self, name):
        if name not in self.sets:
            L = ol.load_set(name)
            K = ol.Keys(L, seed=5)
            idx = self.api.ps_index(name)
            self.api.ps_initialize(idx, K.bk, K.ksk)
            p = self.api.ps_params(idx)
            self.sets[name] = dict(idx=idx, K=K, l=ol.set_params(L)[1]["l"], limbs=p.key_limbs, mu=p.mu, w=K.words, trlwe=(K.k + 1) * K.N)
        return self.sets[name]

    def ps_gates(self, name, level):
        def make():
            K = self.pset(name)["K"]
            ops = np.array([NAND, MUX, NOT, COPY, XOR, NMUX, AND], I32)
            bits = np.random.default_rng(9500 + level).integers(0, 2, size=(3, D)).astype(np.uint8)
            ins = [K.encrypt(bits[i], level, seed=9501 + 10 * level + i) for i in range(3)]
            ins[0][0, :4] = 0
            ins[1][0, :4] = 0
            ins[0][6, :] = 0x7FFFFFFF
            ins[1][6, :] = 0x7FFFFFFF
            return ops, ins, K.gate_batch(ops, level, *ins)
        return self.once(("ps_gates", name, level), make)

    def ps_trlwe(self, name):
        """tl, acc3, acc, seiks, refresh of a set: test_gpu_positions.py::trlwe_ref with D inputs"""
        def make():
            K = self.pset(name)["K"]
            r = dict(tl=_corner_tlwe0(np.random.default_rng(9700), K.n, D))
            r["acc3"] = np.stack(_pmap(lambda d: K.blind_rotate(r["tl"][d], 3), range(D)))
            r["acc"] = np.stack(_pmap(lambda d: K.blind_rotate(r["tl"][d], -1), range(D)))
            r["seiks"] = np.stack(_pmap(lambda d: K.keyswitch(self._extract0(K, r["acc"][d])), range(D)))
            r["refresh"] = np.stack(_pmap(lambda d: K.blind_rotate(r["seiks"][d], -1), range(D)))
            t1 = rnd(4200, (D, K.words[1]))
            t1[0], t1[1] = 0, 0xFFFFFFFF
            r["t1"] = t1
            r["ks"] = np.stack(_pmap(lambda d: K.keyswitch(t1[d]), range(D)))
            return r
        return self.once(("ps_trlwe", name), make)


@pytest.fixture(scope="module")
def env(engine, oracle, keys, keys2, random_words):  # noqa: F811
    e = Env(engine, oracle, keys, keys2, random_words)
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the callables that make the calls: build(env, variant, count, n_call, alias) -> Call.  The arena is laid out for `count` rows and
# the call is made with n_call (== count except in the over-long launches)
# ---------------------------------------------------------------------------------------------------------------------------------
BUILD = {}


def build(f):
    BUILD[f.__name__] = f
    return f


def _host(a, n_call, dtype=I32):
    """a host array of a call: at least one entry, so that its pointer is never null"""
    a = np.ascontiguousarray(a, dtype)
    return a if a.size else np.zeros(max(1, n_call), dtype)


def _gate_operands(words, count, pad, alias, rows=None):
    rows = count if rows is None else rows
    stride = words + pad
    ops = [O("in0", U32, rows, words, "inout" if alias else "in", stride), O("in1", U32, rows, words, "in", stride), O("in2", U32, rows, words, "in", stride)]
    if not alias:
        ops.insert(0, O("out", U32, rows, words, "out", stride))
    return ops


@build
def gate_batch(env, v, count, n_call, alias):
    level, pad = v["level"], v.get("pad", 0)
    words = ol.LVL_WORDS[level]
    ops, ins, want = env.gates(level, count)
    ops = _host(ops, n_call)
    out = "in0" if alias else "out"
    fn = lambda a: env.lib.cufhe_amd_gate_batch(0, None, level, n_call, ops.ctypes.data, 1, a.ptr(out), a.ptr("in0"), a.ptr("in1"), a.ptr("in2"), words + pad)  # noqa: E731
    return Call(_gate_operands(words, count, pad, alias), dict(zip(("in0", "in1", "in2"), ins)), fn, {out: ("full", want)})


@build
def gate_list(env, v, count, n_call, alias):
    """the same list with the rows of every operand scattered inside operands of count + 3 slots"""
    level = v["level"]
    words = ol.LVL_WORDS[level]
    ops, ins, want = env.gates(level, count)
    ops = _host(ops, n_call)
    slots = count + 3
    rng = np.random.default_rng(77 + level + count)
    perms = [rng.permutation(slots)[:count] for _ in range(4)]
    fills = {}
    for i, name in enumerate(("in0", "in1", "in2")):
        h = rnd(80 + i, (slots, words))
        h[perms[i]] = ins[i]
        fills[name] = h

    def fn(a):
        arr = lambda name, p: (ctypes.c_void_p * count)(*[a.ptr(name, int(r)) for r in p])  # noqa: E731
        return env.lib.cufhe_amd_gate_list(0, None, level, n_call, ops.ctypes.data, arr("out", perms[3]), arr("in0", perms[0]), arr("in1", perms[1]),
                                           arr("in2", perms[2]))
    return Call(_gate_operands(words, count, 0, False, rows=slots), fills, fn, {"out": ("at", perms[3], want)}, written={"out": perms[3]})


@build
def blind_rotate_batch(env, v, count, n_call, alias):
    steps = v["steps"]
    fn = lambda a: env.lib.cufhe_amd_blind_rotate_batch(0, None, n_call, a.ptr("tlwe0"), a.ptr("acc"), steps)  # noqa: E731
    return Call([O("tlwe0", U32, count, W0, "in"), O("acc", U32, count, TRLWE, "out")], {"tlwe0": tiled(env.tl7, count)}, fn,
                {"acc": ("tiled", env.acc(steps))})


@build
def bootstrap_batch(env, v, count, n_call, alias):
    fn = lambda a: env.lib.cufhe_amd_bootstrap_batch(0, None, n_call, a.ptr("out"), a.ptr("in"))  # noqa: E731
    return Call([O("out", U32, count, W0, "out"), O("in", U32, count, W0, "in")], {"in": tiled(env.tl7, count)}, fn, {"out": ("tiled", env.seiks)})


@build
def refresh_batch(env, v, count, n_call, alias):
    if alias:
        fn = lambda a: env.lib.cufhe_amd_refresh_batch(0, None, n_call, a.ptr("trlwe"), a.ptr("trlwe"))  # noqa: E731
        return Call([O("trlwe", U32, count, TRLWE, "inout")], {"trlwe": tiled(env.acc(-1), count)}, fn, {"trlwe": ("tiled", env.refresh)})
    fn = lambda a: env.lib.cufhe_amd_refresh_batch(0, None, n_call, a.ptr("trlwe_in"), a.ptr("trlwe_out"))  # noqa: E731
    return Call([O("trlwe_in", U32, count, TRLWE, "in"), O("trlwe_out", U32, count, TRLWE, "out")], {"trlwe_in": tiled(env.acc(-1), count)}, fn,
                {"trlwe_out": ("tiled", env.refresh)})


def _lut(env, v, count, n_call, lookup):
    nout = v["nout"]
    src = _host(tiled(SRC7, count), n_call)
    row = nout * W0 if lookup else TRLWE
    operands = [O("tlwe0", U32, count, W0, "in"), O("tables", U32, D, TRLWE, "in"), O("out", U32, count, row, "out")]
    if lookup:
        fn = lambda a: env.lib.cufhe_amd_lut_lookup_batch(0, None, n_call, a.ptr("tlwe0"), a.ptr("tables"), D, src.ctypes.data, nout, a.ptr("out"))  # noqa: E731
    else:
        fn = lambda a: env.lib.cufhe_amd_lut_rotate_batch(0, None, n_call, a.ptr("tlwe0"), a.ptr("tables"), D, src.ctypes.data, nout, 3, a.ptr("out"))  # noqa: E731
    want = env.lut_lookup(nout) if lookup else env.lut_rotate(nout)
    return Call(operands, {"tlwe0": tiled(env.lut_x, count), "tables": env.tables}, fn, {"out": ("tiled", want)})


@build
def lut_rotate_batch(env, v, count, n_call, alias):
    return _lut(env, v, count, n_call, False)


@build
def lut_lookup_batch(env, v, count, n_call, alias):
    return _lut(env, v, count, n_call, True)


@build
def keyswitch_batch(env, v, count, n_call, alias):
    fn = lambda a: env.lib.cufhe_amd_keyswitch_batch(0, None, n_call, a.ptr("tlwe1"), a.ptr("tlwe0"))  # noqa: E731
    return Call([O("tlwe1", U32, count, W1, "in"), O("tlwe0", U32, count, W0, "out")], {"tlwe1": tiled(env.t1, count)}, fn, {"tlwe0": ("tiled", env.ks)})


@build
def sample_extract_keyswitch_batch(env, v, count, n_call, alias):
    fn = lambda a: env.lib.cufhe_amd_sample_extract_keyswitch_batch(0, None, n_call, a.ptr("trlwe"), a.ptr("tlwe0"))  # noqa: E731
    return Call([O("trlwe", U32, count, TRLWE, "in"), O("tlwe0", U32, count, W0, "out")], {"trlwe": tiled(env.acc(-1), count)}, fn,
                {"tlwe0": ("tiled", env.seiks)})


def _extract_index(env, v, count, n_call, keyswitch):
    shared = v.get("src", True)
    idx = _host(tiled(IDX7, count), n_call)
    src = _host(tiled(SRC7, count), n_call) if shared else None
    rows = D if shared else count
    out = ("tlwe0", W0) if keyswitch else ("tlwe1", W1)
    f = env.lib.cufhe_amd_sample_extract_index_keyswitch_batch if keyswitch else env.lib.cufhe_amd_sample_extract_index_batch
    fn = lambda a: f(0, None, n_call, a.ptr("trlwe"), src.ctypes.data if shared else None, idx.ctypes.data, a.ptr(out[0]))  # noqa: E731
    want = env.extract_ks(shared) if keyswitch else env.extract(shared)
    return Call([O("trlwe", U32, rows, TRLWE, "in"), O(out[0], U32, count, out[1], "out")], {"trlwe": env.trl if shared else tiled(env.trl, count)}, fn,
                {out[0]: ("tiled", want)})


@build
def sample_extract_index_keyswitch_batch(env, v, count, n_call, alias):
    return _extract_index(env, v, count, n_call, True)


@build
def sample_extract_index_batch(env, v, count, n_call, alias):
    return _extract_index(env, v, count, n_call, False)


def _trgsw_to_ntt(env, count, n_call, call, tg, ntt):
    fn = lambda a: call(n_call, a.ptr("trgsw"), a.ptr("trgsw_ntt"))  # noqa: E731
    return Call([O("trgsw", U32, count, tg.shape[1], "in"), O("trgsw_ntt", F64, count, ntt.shape[1], "out")], {"trgsw": tiled(tg, count)}, fn,
                {"trgsw_ntt": ("tiled", ntt)})


def _cmux(env, count, n_call, alias, call, data, ntt):
    tg, c1, c0, want = data
    roles = {"c1": "inout" if alias == "res == c1" else "in", "c0": "inout" if alias == "res == c0" else "in"}
    res = "c1" if alias == "res == c1" else "c0" if alias == "res == c0" else "res"
    operands = [O("trgsw_ntt", F64, count, ntt.shape[1], "in"), O("c1", U32, count, c1.shape[1], roles["c1"]), O("c0", U32, count, c0.shape[1], roles["c0"])]
    if res == "res":
        operands.append(O("res", U32, count, want.shape[1], "out"))
    fn = lambda a: call(n_call, a.ptr("trgsw_ntt"), a.ptr("c1"), a.ptr("c0"), a.ptr(res))  # noqa: E731
    return Call(operands, {"trgsw_ntt": tiled(ntt, count), "c1": tiled(c1, count), "c0": tiled(c0, count)}, fn, {res: ("tiled", want)})


@build
def trgsw_to_ntt_batch(env, v, count, n_call, alias):
    tg = env.cmux_data(env.keys)[0]
    return _trgsw_to_ntt(env, count, n_call, lambda c, s, d: env.lib.cufhe_amd_trgsw_to_ntt_batch(0, None, c, s, d), tg, env.ntt_of("default", tg))


@build
def cmux_batch(env, v, count, n_call, alias):
    data = env.cmux_data(env.keys)
    return _cmux(env, count, n_call, alias, lambda c, g, c1, c0, r: env.lib.cufhe_amd_cmux_batch(0, None, c, g, c1, c0, r), data, env.ntt_of("default", data[0]))


@build
def trlwe_rotate_batch(env, v, count, n_call, alias):
    exps = _host(tiled(EXPS7, n_call), n_call)
    fn = lambda a: env.lib.cufhe_amd_trlwe_rotate_batch(0, None, n_call, a.ptr("in"), exps.ctypes.data, a.ptr("out"))  # noqa: E731
    return Call([O("in", U32, count, TRLWE, "in"), O("out", U32, count, TRLWE, "out")], {"in": tiled(env.trl, count)}, fn, {"out": ("tiled", env.rotate)})


@build
def cmux_rotate_batch(env, v, count, n_call, alias):
    ntt = env.ntt_of("selector", env.selector.reshape(1, TRGSW))
    exps = _host(tiled(EXPS7, count), n_call)
    res = "c" if alias else "res"
    operands = [O("trgsw_ntt", F64, 1, TRGSW, "in"), O("c", U32, count, TRLWE, "inout" if alias else "in")] + ([] if alias else [O("res", U32, count, TRLWE, "out")])
    fn = lambda a: env.lib.cufhe_amd_cmux_rotate_batch(0, None, n_call, a.ptr("trgsw_ntt"), exps.ctypes.data, a.ptr("c"), a.ptr(res))  # noqa: E731
    return Call(operands, {"trgsw_ntt": ntt, "c": tiled(env.trl, count)}, fn, {res: ("tiled", env.cmux_rotate)})


def _polymul(env, count, n_call, f, data):
    a, b, want = data
    fn = lambda ar: f(0, None, n_call, ar.ptr("a"), ar.ptr("b"), ar.ptr("res"))  # noqa: E731
    m = a.shape[1]
    return Call([O("a", I32, count, m, "in"), O("b", U32, count, m, "in"), O("res", U32, count, m, "out")], {"a": tiled(a, count), "b": tiled(b, count)}, fn,
                {"res": ("tiled", want)})


@build
def polymul_batch(env, v, count, n_call, alias):
    return _polymul(env, count, n_call, env.lib.cufhe_amd_polymul_batch, env.poly)


@build
def polymul512_batch(env, v, count, n_call, alias):
    return _polymul(env, count, n_call, env.lib.cufhe_amd_polymul512_batch, env.poly512)


@build
def trlwe_spread_batch(env, v, count, n_call, alias):
    stride, reps = v["stride"], v["reps"]
    fn = lambda a: env.lib.cufhe_amd_trlwe_spread_batch(0, None, n_call, a.ptr("in"), stride, reps, a.ptr("out"))  # noqa: E731
    return Call([O("in", U32, count, TRLWE, "in"), O("out", U32, count, TRLWE, "out")], {"in": tiled(env.trl, count)}, fn,
                {"out": ("tiled", env.spread(stride, reps))})


@build
def lvl2_gate_batch(env, v, count, n_call, alias):
    ops7, ins, want = env.ring_gates
    ops = _host(tiled(ops7, count), n_call)
    fn = lambda a: env.lib.cufhe_amd_lvl2_gate_batch(0, None, n_call, ops.ctypes.data, 1, a.ptr("out"), a.ptr("in0"), a.ptr("in1"), a.ptr("in2"), W0)  # noqa: E731
    return Call(_gate_operands(W0, count, 0, False), {k: tiled(x, count) for k, x in zip(("in0", "in1", "in2"), ins)}, fn, {"out": ("first", want)})


@build
def lvl2_blind_rotate_batch(env, v, count, n_call, alias):
    steps = v["steps"]
    fn = lambda a: env.lib.cufhe_amd_lvl2_blind_rotate_batch(0, None, n_call, a.ptr("tlwe0"), a.ptr("acc"), steps)  # noqa: E731
    return Call([O("tlwe0", U32, count, W0, "in"), O("acc", U64, count, 2 * N2, "out")], {"tlwe0": tiled(env.tl7, count)}, fn,
                {"acc": ("tiled", env.acc2(steps))})


@build
def lvl2_user_rotate_batch(env, v, count, n_call, alias):
    fn = lambda a: env.lib.cufhe_amd_lvl2_user_rotate_batch(0, None, n_call, env.op2["one"], a.ptr("in0"), None, None, 2, a.ptr("acc"))  # noqa: E731
    return Call([O("in0", U32, count, W0, "in"), O("acc", U64, count, 2 * N2, "out")], {"in0": tiled(env.tl7, count)}, fn,
                {"acc": ("tiled", env.user_rotate2)})


@build
def lvl2_user_extract_batch(env, v, count, n_call, alias):
    _, ins, _ = env.ring_gates
    fn = lambda a: env.lib.cufhe_amd_lvl2_user_extract_batch(0, None, n_call, env.op2["three"], a.ptr("in0"), a.ptr("in1"), a.ptr("in2"), a.ptr("tlwe2"))  # noqa: E731
    operands = [O(k, U32, count, W0, "in") for k in ("in0", "in1", "in2")] + [O("tlwe2", U64, count, W2, "out")]
    return Call(operands, {k: tiled(x, count) for k, x in zip(("in0", "in1", "in2"), ins)}, fn, {"tlwe2": ("first", env.user_extract2)})


@build
def lvl2_keyswitch_batch(env, v, count, n_call, alias):
    fn = lambda a: env.lib.cufhe_amd_lvl2_keyswitch_batch(0, None, n_call, a.ptr("tlwe2"), a.ptr("tlwe0"))  # noqa: E731
    return Call([O("tlwe2", U64, count, W2, "in"), O("tlwe0", U32, count, W0, "out")], {"tlwe2": tiled(env.t2, count)}, fn, {"tlwe0": ("tiled", env.ks2)})


@build
def cb_rotate_batch(env, v, count, n_call, alias):
    fn = lambda a: env.lib.cufhe_amd_cb_rotate_batch(0, None, n_call, a.ptr("tlwe0"), a.ptr("tlwe2"))  # noqa: E731
    return Call([O("tlwe0", U32, count, W0, "in"), O("tlwe2", U64, count, cb.CB_L * W2, "out")], {"tlwe0": tiled(env.tl7, count)}, fn,
                {"tlwe2": ("first", env.stage1.reshape(RING_ROWS, cb.CB_L * W2))})


@build
def private_keyswitch_batch(env, v, count, n_call, alias):
    fn = lambda a: env.lib.cufhe_amd_private_keyswitch_batch(0, None, n_call, a.ptr("tlwe2"), a.ptr("trlwe"))  # noqa: E731
    return Call([O("tlwe2", U64, count, W2, "in"), O("trlwe", U32, count, 2 * TRLWE, "out")], {"tlwe2": tiled(env.pks_in, count)}, fn,
                {"trlwe": ("tiled", env.pks)})


@build
def circuit_bootstrap_batch(env, v, count, n_call, alias):
    outs = v["outs"]
    operands = [O("tlwe0", U32, count, W0, "in")]
    want = {}
    if "trgsw" in outs:
        operands.append(O("trgsw", U32, count, TRGSW, "out"))
        want["trgsw"] = ("first", env.cb_trgsw)
    if "trgsw_ntt" in outs:
        operands.append(O("trgsw_ntt", F64, count, TRGSW, "out"))
        want["trgsw_ntt"] = ("first", env.ntt_of("cb", env.cb_trgsw))
    fn = lambda a: env.lib.cufhe_amd_circuit_bootstrap_batch(0, None, n_call, a.ptr("tlwe0"), a.ptr("trgsw") if "trgsw" in outs else None,  # noqa: E731
                                                             a.ptr("trgsw_ntt") if "trgsw_ntt" in outs else None)
    return Call(operands, {"tlwe0": tiled(env.tl7, count)}, fn, want)


def pack_targets(count, count_out):
    """dst / pos of `count` inputs, as tests/test_gpu_pack.py::targets: with 5 outputs, output 3 stays unnamed, output 1 is named by
    every second input and the others share 0, 2 and 4; the positions cycle through 0, 1, N - 1 and 511"""
    dst = np.zeros(count, I32)
    if count_out > 1:
        others = [o for o in range(count_out) if o not in (1, 3)]
        dst[:] = [1 if m % 2 else others[(m // 2) % len(others)] for m in range(count)]
    p = np.array([(0, 1, N - 1, 511)[m % 4] for m in range(count)], I32)
    if count >= 2:
        dst[-1], p[-1] = dst[0], p[0]
    return dst, p


@build
def pack_batch(env, v, count, n_call, alias):
    count_out = v["count_out"]
    x7, rows7 = env.pack_rows
    dst, p = pack_targets(count, count_out)
    want = np.zeros((count_out, TRLWE), U32)
    for m in range(count):
        want[dst[m]] += pk.rotate(rows7[m % D], int(p[m]))
    hd, hp = _host(dst, n_call), _host(p, n_call)
    fn = lambda a: env.lib.cufhe_amd_pack_batch(0, None, n_call, a.ptr("tlwe0"), hd.ctypes.data, hp.ctypes.data, count_out, a.ptr("trlwe"))  # noqa: E731
    return Call([O("tlwe0", U32, count, W0, "in"), O("trlwe", U32, count_out, TRLWE, "out")], {"tlwe0": tiled(x7, count)}, fn, {"trlwe": ("full", want)})


def _ps_gate(env, v, count, n_call, level, by_level):
    s = env.pset(v["set"])
    ops7, ins, want = env.ps_gates(v["set"], level)
    ops = _host(tiled(ops7, count), n_call)
    words = s["w"][level]
    if by_level:
        fn = lambda a: env.lib.cufhe_amd_ps_gate_batch_level(s["idx"], 0, None, level, n_call, ops.ctypes.data, 1, a.ptr("out"), a.ptr("in0"), a.ptr("in1"),  # noqa: E731
                                                             a.ptr("in2"), words)
    else:
        fn = lambda a: env.lib.cufhe_amd_ps_gate_batch(s["idx"], 0, None, n_call, ops.ctypes.data, 1, a.ptr("out"), a.ptr("in0"), a.ptr("in1"), a.ptr("in2"), words)  # noqa: E731
    return Call(_gate_operands(words, count, 0, False), {k: tiled(x, count) for k, x in zip(("in0", "in1", "in2"), ins)}, fn, {"out": ("tiled", want)})


@build
def ps_gate_batch(env, v, count, n_call, alias):
    return _ps_gate(env, v, count, n_call, 0, False)


@build
def ps_gate_batch_level(env, v, count, n_call, alias):
    return _ps_gate(env, v, count, n_call, v["level"], True)


@build
def ps_blind_rotate_batch(env, v, count, n_call, alias):
    s, r = env.pset(v["set"]), env.ps_trlwe(v["set"])
    fn = lambda a: env.lib.cufhe_amd_ps_blind_rotate_batch(s["idx"], 0, None, n_call, a.ptr("tlwe0"), a.ptr("acc"), 3)  # noqa: E731
    return Call([O("tlwe0", U32, count, s["w"][0], "in"), O("acc", U32, count, s["trlwe"], "out")], {"tlwe0": tiled(r["tl"], count)}, fn,
                {"acc": ("tiled", r["acc3"])})


@build
def ps_keyswitch_batch(env, v, count, n_call, alias):
    s, r = env.pset(v["set"]), env.ps_trlwe(v["set"])
    fn = lambda a: env.lib.cufhe_amd_ps_keyswitch_batch(s["idx"], 0, None, n_call, a.ptr("tlwe1"), a.ptr("tlwe0"))  # noqa: E731
    return Call([O("tlwe1", U32, count, s["w"][1], "in"), O("tlwe0", U32, count, s["w"][0], "out")], {"tlwe1": tiled(r["t1"], count)}, fn,
                {"tlwe0": ("tiled", r["ks"])})


@build
def ps_trgsw_to_ntt_batch(env, v, count, n_call, alias):
    s = env.pset(v["set"])
    tg = env.cmux_data(s["K"])[0]
    ntt = env.ntt_of(v["set"], tg, ps=s["idx"], limbs=s["limbs"])
    return _trgsw_to_ntt(env, count, n_call, lambda c, a, d: env.lib.cufhe_amd_ps_trgsw_to_ntt_batch(s["idx"], 0, None, c, a, d), tg, ntt)


@build
def ps_cmux_batch(env, v, count, n_call, alias):
    s = env.pset(v["set"])
    data = env.cmux_data(s["K"])
    ntt = env.ntt_of(v["set"], data[0], ps=s["idx"], limbs=s["limbs"])
    return _cmux(env, count, n_call, alias, lambda c, g, c1, c0, r: env.lib.cufhe_amd_ps_cmux_batch(s["idx"], 0, None, c, g, c1, c0, r), data, ntt)


@build
def ps_trlwe_op_batch(env, v, count, n_call, alias):
    s, r = env.pset(v["set"]), env.ps_trlwe(v["set"])
    op, src, dst, iw, ow = {"bootstrap": (env.api.TL_BOOTSTRAP, "tl", "acc", s["w"][0], s["trlwe"]),
                            "refresh": (env.api.TL_REFRESH, "acc", "refresh", s["trlwe"], s["trlwe"]),
                            "seiks": (env.api.TL_SEIKS, "acc", "seiks", s["trlwe"], s["w"][0])}[v["op"]]
    fn = lambda a: env.lib.cufhe_amd_ps_trlwe_op_batch(s["idx"], 0, None, op, n_call, a.ptr("out"), a.ptr("in"))  # noqa: E731
    return Call([O("out", U32, count, ow, "out"), O("in", U32, count, iw, "in")], {"in": tiled(r[src], count)}, fn, {"out": ("tiled", r[dst])})


# ---------------------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------------------
def options_of(variant):
    opts = dict(SHAPES[variant["shape"]]) if "shape" in variant else {}
    opts.update(variant["opts"])
    return opts


def launch(env, symbol, variant, count, n_call=None, alias=None):
    """arena, its words after the call, the status, the Call"""
    n_call = count if n_call is None else n_call
    call = BUILD[fp.CASES[symbol].build](env, variant, count, n_call, alias)
    label = f"{symbol[len('cufhe_amd_'):]} [{variant['id']}{', ' + alias if alias else ''}], count {n_call}"
    arena = fp.Arena(label, call.operands, DeviceBackend(env.api))
    try:
        for name, rows in call.fills.items():
            arena.set(name, rows)
        for name, rows in call.written.items():
            arena.written(name, rows)
        arena.upload()
        with pos.options(env.api, options_of(variant)):
            rc = call.fn(arena)
            sync = env.lib.cufhe_amd_synchronize()
        after = arena.download()
    finally:
        arena.backend.buf.free()
    if rc == -2 or sync != 0:
        # a HIP call failed: nothing more is started on the device
        pytest.exit(f"{label}: status {rc}, synchronize {sync}: {env.lib.cufhe_amd_last_error().decode()}", returncode=3)
    return arena, after, rc, call


def compare(arena, after, call, label):
    for name, want in call.want.items():
        got = arena.rows(after, name)
        if want[0] == "tiled":
            if got.shape[0]:
                pos.assert_every_row(got, want[1], f"{label}, {name}")
        else:
            rows = got if want[0] in ("full", "first") else got[want[1]]
            assert want[0] != "first" or rows.shape[0] <= RING_ROWS
            expect = np.ascontiguousarray(want[-1][:rows.shape[0]] if want[0] == "first" else want[-1]).reshape(rows.shape)
            bad = np.flatnonzero((rows != expect).any(axis=1))
            assert bad.size == 0, f"{label}, {name}: rows {bad[:10].tolist()} differ from the reference"


def run(env, symbol, variant, count, alias=None):
    arena, after, rc, call = launch(env, symbol, variant, count, alias=alias)
    assert rc == 0, f"{arena.label}: status {rc}: {env.lib.cufhe_amd_last_error().decode()}"
    compare(arena, after, call, arena.label)
    msg = arena.check(after)
    assert msg is None, msg
    if count == 0 and symbol != "cufhe_amd_pack_batch":
        assert np.array_equal(after, arena.before), f"{arena.label}: an empty batch changed the arena"


RUNS = [(sym, rid, v, c) for sym, case in fp.CASES.items() for rid, v, c in case.runs()]


@pytest.mark.parametrize("symbol,variant,count", [pytest.param(s, v, c, id=f"{s[len('cufhe_amd_'):]}-{rid}") for s, rid, v, c in RUNS])
def test_footprint(env, symbol, variant, count):
    run(env, symbol, variant, count)


def _first_variant(symbol):
    return fp.CASES[symbol].variants[0]


PERMITTED = [(s, a) for s, case in fp.CASES.items() for a in case.permitted]


@pytest.mark.parametrize("symbol,alias", PERMITTED, ids=[f"{s[len('cufhe_amd_'):]}-{a.replace(' ', '')}" for s, a in PERMITTED])
def test_permitted_aliasing(env, symbol, alias):
    """every overlap the header permits, at U + 1: the aliased operand is inout and holds the words of the non-aliased run"""
    case = fp.CASES[symbol]
    for v in case.variants[:1] if not symbol.startswith("cufhe_amd_ps_") else [x for x in case.variants if x["id"] in fp.PS_CMUX_SETS]:
        u = case.unit(v)
        run(env, symbol, v, u + 1 if u > 1 else 3, alias=alias)


@pytest.mark.parametrize("symbol", [s for s, case in fp.CASES.items() if case.forbidden])
def test_forbidden_overlap(env, symbol):
    """out overlapping in -- the same rows, and shifted by one row and by one word -- returns -1 and leaves every arena word as it was"""
    case = fp.CASES[symbol]
    v = _first_variant(symbol)
    count = case.unit(v) + 1
    call = BUILD[case.build](env, v, count, count, None)
    for shift_words in (0, TRLWE, 1, count * TRLWE - 1):
        arena = fp.Arena(f"{symbol}, out = in + {shift_words} words", [O("in", U32, count, TRLWE, "in")], DeviceBackend(env.api))
        try:
            arena.set("in", call.fills["in"])
            arena.upload()
            out = arena.ptr("in") + 4 * shift_words
            if symbol == "cufhe_amd_trlwe_rotate_batch":
                exps = tiled(EXPS7, count)
                rc = env.lib.cufhe_amd_trlwe_rotate_batch(0, None, count, arena.ptr("in"), exps.ctypes.data, out)
            else:
                rc = env.lib.cufhe_amd_trlwe_spread_batch(0, None, count, arena.ptr("in"), v["stride"], v["reps"], out)
            assert env.lib.cufhe_amd_synchronize() == 0
            after = arena.download()
        finally:
            arena.backend.buf.free()
        assert rc == -1, f"{arena.label}: status {rc}"
        assert np.array_equal(after, arena.before), arena.check(after) or f"{arena.label}: the arena changed"


OVERLONG_VARIANT = {
    "cufhe_amd_blind_rotate_batch": lambda: next(v for v in fp.CASES["cufhe_amd_blind_rotate_batch"].variants if v["shape"] == "batch" and v["steps"] == 1),
    "cufhe_amd_keyswitch_batch": lambda: next(v for v in fp.CASES["cufhe_amd_keyswitch_batch"].variants if v["id"] == "16x2"),
    "cufhe_amd_trlwe_rotate_batch": lambda: _first_variant("cufhe_amd_trlwe_rotate_batch"),
}


@pytest.mark.parametrize("symbol", fp.OVERLONG)
def test_harness_sees_a_launch_of_one_row_too_many(env, symbol):
    """The arena is laid out for `count` rows and the call is made with count + 1: a deliberate over-long batch inside owned memory
    (the guards hold two rows behind every operand, inputs included; guard words are valid ciphertext words).  Arena.check must
    report exactly one extra row directly after the output's last row, and nothing else."""
    case = fp.CASES[symbol]
    v = OVERLONG_VARIANT[symbol]()
    count = case.unit(v) + 1
    arena, after, rc, call = launch(env, symbol, v, count, n_call=count + 1)
    assert rc == 0, f"{arena.label}: status {rc}: {env.lib.cufhe_amd_last_error().decode()}"
    compare(arena, after, call, arena.label)
    (name,) = call.want
    o = arena[name]
    assert o.back_guard >= 2 * o.row_words
    found = arena.findings(after)
    assert len(found) == 1, arena.check(after)
    f = found[0]
    assert (f["operand"], f["side"], f["distance"], f["words"]) == (name, "after", 0, o.row_elems), arena.check(after)
    assert f"{name}: {o.row_elems} words changed starting 0 words after the last row (= row `count`)" in arena.check(after)
