"""The stream contract of the batch entry points (include/cufhe_amd.h, "Streams"), where a caller meets it:

  1. chains of dependent calls on ONE created stream with no host synchronise in between, their counts falling and rising so that the
     stream's workspace, the digit words of the matrix key switch and the temporary of linear_gate_batch are regrown while earlier
     work is in flight and reused shrunk afterwards (tests/stream_contract.py has the arithmetic);
  2. host argument arrays overwritten with OTHER VALID values the moment their call returns, behind 1024 bootstraps that keep the
     stream busy;
  3. two and four streams, and a stream beside the null stream, with such chains in flight together, issued alternately from one
     thread;
  4. two issuing threads, a stream each;
  5. stream_destroy without a synchronise, the handle reused, and the device memory the library pooled for the stream.

Every expected word comes from the CPU checkers (the oracle, user_gate_checker, packed_rom_checker, pack_checker, lut_checker,
linear_checker, cb_checker), never from a GPU run.  Batches are tiled from D = 7 distinct inputs as in tests/positions.py: the reference
is computed for 7 rows per call and every row of every buffer is compared.  A lane (one stream's sequence) lays all its buffers out
in ONE footprint.Arena: outputs are poisoned, a buffer that a larger later call reads past the rows its producer writes holds the
producer's expected words there, and after the single synchronise the whole arena is checked for stray stores.

A device error ends the session (pytest.exit): nothing more runs on a card that has faulted.
"""
import ctypes
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import cb_checker as cb
import footprint as fp
import linear_checker as lin
import lut_checker as lc
import lvl2_multi_checker as l2m
import lvl2_user_gate_checker as l2c
import oracle_lib as ol
import pack_checker as pk
import packed_rom_checker as prc
import positions as pos
import stream_contract as sc
import user_gate_checker as uc

pytestmark = pytest.mark.gpu

N, n = ol.N, ol.n
W0, W1, TR = n + 1, N + 1, 2 * N
TRGSW = 2 * 3 * 2 * N                     # torus words of one TRGSW; its NTT form is as many doubles
D = 7
U32 = np.uint32
OPS = {name: i for i, name in enumerate(ol.OPS)}
KS_KERNELS = {       # the option sets that put every lvl10 key switch of a launch on one kernel (plan::plan_keyswitch, use_matrix_keyswitch)
    "matrix": dict(ks_mm_threshold=1),
    "split8": dict(ks_mm_threshold=0, ks_split_threshold=1 << 30),                                # zeroing kernel, then eight adding workgroups
    "workgroup": dict(ks_mm_threshold=0, ks_split_threshold=0, ks_wg_threshold=1 << 30),
    "shared": dict(ks_mm_threshold=0, ks_split_threshold=0, ks_wg_threshold=0, ks_per_wg=6, ks_slices=1),
    "sliced": dict(ks_mm_threshold=0, ks_split_threshold=0, ks_wg_threshold=0, ks_per_wg=16, ks_slices=64),   # zeroing kernel, then atomic adds
}
assert pos.check_period(D) is None and sc.W0 == W0 and sc.W1 == W1


def rnd(seed, *shape):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(U32)


def pmap(fn, count):
    """fn(0) alone first (the oracle builds its tables once), the rest on threads: ctypes releases the GIL"""
    first = [fn(0)]
    with ThreadPoolExecutor(16) as ex:
        return np.stack(first + list(ex.map(fn, range(1, count))))


def device_call(eng, fn, what):
    """a library call; status -2 (a HIP error) ends the session"""
    try:
        return fn()
    except eng.CufheAmdError as e:
        if "error -2" in str(e):
            pytest.exit(f"{what}: {e}", returncode=3)
        raise


def synchronize(eng, st, what):
    rc = eng.lib.cufhe_amd_stream_synchronize(0, st)
    if rc != 0:
        pytest.exit(f"{what}: stream synchronise returned {rc}: {eng.lib.cufhe_amd_last_error().decode()}", returncode=3)


class DeviceBackend:
    def __init__(self, api):
        self.api = api

    def alloc(self, words):
        self.buf = self.api.DeviceBuffer(words)
        return self.buf.ptr

    def upload(self, host):
        self.buf.upload(host)

    def download(self):
        return self.buf.download()


# ---------------------------------------------------------------------------------------------------------------------------------
# a lane: the calls of one stream and the arena they run in
# ---------------------------------------------------------------------------------------------------------------------------------
class Lane:
    def __init__(self, eng, label, stream):
        self.eng, self.api, self.label, self.st = eng, eng.api, label, stream
        self.specs, self.calls, self.checks, self.arena = [], [], [], None

    # -- declaration
    def inp(self, name, rows_words):
        a = np.ascontiguousarray(rows_words)
        self.specs.append(dict(name=name, dtype=a.dtype, rows=a.shape[0], elems=int(np.prod(a.shape[1:])), role="in", host=a, live=None))

    def out(self, name, want, live, rows=None):
        """`live` rows that one call writes (poisoned before); rows past them, read by a larger later call, hold the expected words.
        want: [D][...] -- row g must come out as want[g % D]."""
        want = np.ascontiguousarray(want)
        rows = max(live, rows or 0)
        host = pos.tile(want, rows).reshape(rows, -1)
        host[:live] = pos.poison((live, host.shape[1]), want.dtype)
        self.specs.append(dict(name=name, dtype=want.dtype, rows=rows, elems=host.shape[1], role="inout", host=host, live=live))
        self.checks.append((name, live, want))

    def call(self, what, fn):
        self.calls.append((what, fn))

    # -- device
    def build(self):
        ops = [fp.Operand(s["name"], s["dtype"], s["rows"], s["elems"], s["role"]) for s in self.specs]
        self.arena = fp.Arena(self.label, ops, DeviceBackend(self.api))
        for s in self.specs:
            self.arena.set(s["name"], s["host"].reshape(s["rows"], s["elems"]))
            if s["live"] is not None:
                self.arena.written(s["name"], np.arange(s["live"]))
        self.arena.upload()
        return self

    def reset(self):
        self.arena.upload()

    def v(self, name, row=0):
        """what the api takes for a device array: the operand from `row` on"""
        o = self.arena[name]
        return fp.View(self.arena.ptr(name, row), (o.rows - row) * o.row_words)

    def issue(self, i):
        what, fn = self.calls[i]
        device_call(self.eng, fn, f"{self.label}: {what}")

    def sync(self):
        synchronize(self.eng, self.st, self.label)

    def failures(self):
        after = self.arena.download()
        out = []
        msg = self.arena.check(after)
        if msg:
            out.append(msg)
        for name, live, want in self.checks:
            got = self.arena.rows(after, name)[:live].reshape((live,) + want.shape[1:])
            msg = pos.report(np.ascontiguousarray(got), want, f"{self.label}: {name}, {live} rows")
            if msg:
                out.append(msg)
        return out

    def close(self):
        if self.arena is not None:
            self.arena.backend.buf.free()
            self.arena = None


def run_lanes(lanes):
    """A1 B1 A2 B2 ... from this thread, no synchronise until every call is issued; then every stream, then every word"""
    try:
        for lane in lanes:
            lane.build()
        for k, i in sc.round_robin([len(lane.calls) for lane in lanes]):
            lanes[k].issue(i)
        for lane in lanes:
            lane.sync()
        bad = [m for lane in lanes for m in lane.failures()]
    finally:
        for lane in lanes:
            lane.close()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# the library state and the references, shared by the module
# ---------------------------------------------------------------------------------------------------------------------------------
class World:
    """user gates, layers and the packing key defined once; the references of every (chain, variant) computed on first use"""

    def __init__(self, eng, keys):
        self.eng, self.api, self.keys = eng, eng.api, keys
        self.user2 = dict(c=(1, -1, 0), off=0x12345678, tv=rnd(7001, N))                 # reads two operands
        self.user1 = dict(c=(3, 0, 0), off=0x0BADF00D, tv=rnd(7002, N))                  # reads one: the activation of linear_gate_batch
        for u in (self.user2, self.user1):
            u["op"] = eng.define_gate(u["c"], u["off"], u["tv"])
        self.pack_key = rnd(7003, pk.KEY_WORDS)
        self.api.pack_initialize(self.pack_key)
        rng = np.random.default_rng(7004)
        self.W1m, self.b1 = lin.test_weights(rng, 3, 2), lin.random_words(rng, 3)
        self.W2m, self.b2 = lin.test_weights(rng, 3, 3), lin.random_words(rng, 3)
        self.W2m[2, :] = (5, -7, 1 << 30)                                                # no zero row in front of the activation
        self.layer1, self.layer2 = eng.define_linear(self.W1m, self.b1), eng.define_linear(self.W2m, self.b2)
        self.streams, self.cache = [], {}
        self.ring = self.pks_key = self.ps = self.user_ring = None

    def stream(self):
        st = self.api.Stream(0)
        st.Create()
        self.streams.append(st)
        return st

    def destroy_streams(self):
        for st in self.streams:
            if st.st():
                st.Destroy()
        self.streams = []

    def ref(self, kind, v):
        if (kind, v) not in self.cache:
            self.cache[kind, v] = getattr(self, "ref_" + kind)(v)
        return self.cache[kind, v]

    # -- the gate chain
    def ref_gate(self, v):
        K, s = self.keys, 7100 + 100 * v
        r = dict(a=rnd(s, D, W0), b=rnd(s + 1, D, W0), c=rnd(s + 2, D, W0), l1a=rnd(s + 3, D, W1), l1b=rnd(s + 4, D, W1), T=rnd(s + 5, D, TR))
        r["a"][0, :4] = 0                                        # a run of abar = 0 in front of the first rotation
        two = [OPS[x] for x in ("NAND", "XOR", "NOR", "XNOR", "AND", "ANDYN", "OR")]
        r["ops1"] = np.array([two[(d + v) % 2] for d in range(D)], np.int32)              # NAND and XOR mixed
        r["x1"] = K.gate_batch(r["ops1"], 0, r["a"], r["b"])
        u = self.user2
        r["ops2"] = np.array([u["op"] if d % 2 == 0 else OPS["MUX"] for d in range(D)], np.int32)

        def second(d):
            if d % 2 == 0:
                return uc.user_gate_one(K, 0, u["c"], u["off"], u["tv"], [r["x1"][d], r["b"][d]])
            return K.gate_batch(OPS["MUX"], 0, r["x1"][d][None], r["b"][d][None], r["c"][d][None], threads=1)[0]
        r["x2"] = pmap(second, D)

        def extract(acc):
            t = np.zeros(W1, U32)
            K.L.orc_sample_extract0(t, np.ascontiguousarray(acc))
            return t
        r["x3"] = pmap(lambda d: K.keyswitch(extract(K.blind_rotate(r["x2"][d]))), D)      # bootstrap_batch
        r["r3"] = pmap(lambda d: K.blind_rotate(K.keyswitch(extract(r["T"][d]))), D)      # refresh_batch
        r["x4"] = pmap(lambda d: K.keyswitch(extract(r["r3"][d])), D)                     # sample_extract_keyswitch_batch
        r["ops5"] = np.array([two[2 + (d + v) % 5] for d in range(D)], np.int32)
        r["y5"] = K.gate_batch(r["ops5"], 1, r["l1a"], r["l1b"])
        r["x6"] = pmap(lambda d: K.keyswitch(r["y5"][d]), D)                              # keyswitch_batch
        r["x7"] = K.gate_batch(OPS["NAND"], 0, r["x6"], r["a"])
        return r

    # -- the TRLWE chain
    STRIDE, REPS = 4, 8

    def ref_trlwe(self, v):
        K, s = self.keys, 7500 + 100 * v
        r = dict(tg=rnd(s, D, TRGSW), c1=rnd(s + 1, D, TR), c0=rnd(s + 2, D, TR), addr=rnd(s + 3, D, W0))
        r["tg"][1] = prc.selector(K, 1)                          # a genuine TRGSW of a key bit among the random ones
        rng = np.random.default_rng(s + 4)
        r["e3"] = np.array([0, 1, 1023, 1024, 1025, 2047, 64][v:] + [0, 1, 1023, 1024, 1025, 2047, 64][:v], np.int32)
        r["e4"] = rng.integers(0, 2 * N, D).astype(np.int32)
        r["idx5"] = np.array([0, 1, 63, 64, 511, 1022, 1023], np.int32)[rng.permutation(D)]
        r["pos6"] = rng.integers(0, N, 2 * D).astype(np.int32)
        r["r2"] = pmap(lambda d: prc.cmux(K.L, r["tg"][d], r["c1"][d], r["c0"][d]), D)
        r["r3"] = pmap(lambda d: prc.cmux_rotate(K.L, r["tg"][0], r["r2"][d], int(r["e3"][d])), D)      # ONE selector for the launch: row 0
        r["r4"] = np.stack([prc.rotate(r["r3"][d], int(r["e4"][d])) for d in range(D)])
        r["x5"] = pmap(lambda d: prc.extract_keyswitch(K, r["r4"][d], int(r["idx5"][d])), D)
        # output o sums the inputs 2 o and 2 o + 1, at positions pos6[2 o mod 2 D], pos6[(2 o + 1) mod 2 D]: period D in o (D is odd)
        r["p6"] = np.stack([self.pack_pair(r["x5"], r["pos6"], d) for d in range(D)])
        r["s7"] = np.stack([lc.spread(r["p6"][d], self.STRIDE, self.REPS) for d in range(D)])
        r["o8"] = pmap(lambda d: lc.lut_lookup(K, r["addr"][d], r["s7"][d], 2), D)         # [D][2][W0]
        return r

    def pack_pair(self, x5, pos6, o):
        ins = np.stack([x5[(2 * o) % D], x5[(2 * o + 1) % D]])
        return pk.pack_batch(self.pack_key, ins, [0, 0], [pos6[(2 * o) % (2 * D)], pos6[(2 * o + 1) % (2 * D)]], 1)[0]

    # -- the linear chain: a set is a row of the arena
    def ref_linear(self, v):
        K, s, u = self.keys, 7900 + 100 * v, self.user1
        r = dict(x=rnd(s, D, 2, W0), bb=rnd(s + 1, D, 3, W0))
        r["y1"] = lin.linear(self.W1m, self.b1, r["x"])                                    # [D][3][W0]
        z = lin.linear(self.W2m, self.b2, r["y1"])
        r["y2"] = pmap(lambda i: uc.user_gate_one(K, 0, u["c"], u["off"], u["tv"], [z[i // 3][i % 3]]), 3 * D).reshape(D, 3, W0)
        r["g3"] = K.gate_batch(OPS["NAND"], 0, r["y2"].reshape(3 * D, W0), r["bb"].reshape(3 * D, W0)).reshape(D, 3, W0)
        return r

    # -- key switches alone
    def ref_ks(self, v):
        y = rnd(8300 + v, D, W1)
        y[0], y[1] = 0, 0xFFFFFFFF
        return dict(y=y, x=pmap(lambda d: self.keys.keyswitch(y[d]), D))

    # -- the N = 2048 ring
    def need_ring(self, oracle):
        if self.ring is None:
            self.ring = ol.KeysLvl2(oracle, self.keys, seed=7)
            self.api.lvl2_initialize(self.ring.bk, self.ring.ksk)
        return self.ring

    def ref_ring(self, v):
        K2, s = self.ring, 8500 + 100 * v
        r = dict(a=rnd(s, D, W0), b=rnd(s + 1, D, W0))
        r["ops1"] = np.array([OPS["NAND"] if (d + v) % 2 else OPS["XOR"] for d in range(D)], np.int32)
        r["ops2"] = np.array([OPS["OR"] if d % 3 else OPS["ANDNY"] for d in range(D)], np.int32)
        r["x1"] = K2.gate_batch(r["ops1"], r["a"], r["b"])
        r["x2"] = K2.gate_batch(r["ops2"], r["x1"], r["b"])
        return r

    # -- circuit bootstrapping: a checker rotation of the ring costs a second or two, so each reference below is 7 to 21 of them on
    #    threads, computed on first use
    def need_ring_gate(self, oracle):
        self.need_ring(oracle)
        if self.user_ring is None:
            tv = np.random.default_rng(8601).integers(0, 2**64, size=ol.N2, dtype=np.uint64)
            self.user_ring = dict(c=(1, -1, 0), off=0x31415926, tv=tv)
            self.user_ring["op"] = self.api.lvl2_define_gate(self.user_ring["c"], self.user_ring["off"], tv)
        return self.user_ring

    def ref_extract(self, v):
        """lvl2_user_extract_batch -> private_keyswitch_batch"""
        u, s = self.user_ring, 8600 + 10 * v
        r = dict(a=rnd(s + 2, D, W0), b=rnd(s + 3, D, W0))
        r["t2"] = np.stack(l2c.on_threads(lambda d: l2c.user_extract_one(self.ring, u["c"], u["off"], u["tv"], [r["a"][d], r["b"][d]]), D))
        r["out"] = cb.private_keyswitch_batch(self.pks_key, r["t2"]).reshape(D, 2 * TR)
        return r

    def ref_cb(self, rotations):
        """circuit_bootstrap_batch (torus and NTT words) -> cmux_batch with the new selectors; `rotations`: the "cb_rotations" setting"""
        s = 8800 + rotations
        # "cb_rotations" 1: seven distinct inputs, one checker rotation each.  3: a 64-bit rotation of the checker is 630 CMux steps in Python,
        # some seconds that threads do not shorten, and an input costs three: the period of seven rows holds THREE distinct inputs (rows
        # 0 1 2 0 1 2 1: neighbours differ, also across the wrap), nine rotations on threads.  Call k of the chain starts at row k of the
        # inputs (cb_chain), so successive calls leave different words in the same place of the workspace and of their outputs.
        uniq, pattern = (rnd(s, D, W0), np.arange(D)) if rotations == 1 else (rnd(s, 3, W0), np.array([0, 1, 2, 0, 1, 2, 1]))
        uniq[0, n] = 0                                           # bbar = 2 N2
        r = dict(x=uniq[pattern], c1=rnd(s + 1, D, TR), c0=rnd(s + 2, D, TR))
        if rotations == 3:       # cb.cb_rotate_one with its three rotations on threads (cb.cb_rotate_batch runs them one after another)
            def row(i):
                t2 = cb.sample_extract0(self.ring, cb.blind_rotate_mu(self.ring, uniq[i // cb.CB_L], cb.cb_mu(i % cb.CB_L)))
                with np.errstate(over="ignore"):
                    t2[ol.N2] += np.uint64(cb.cb_mu(i % cb.CB_L))
                return t2
            stage1 = np.stack(l2c.on_threads(row, cb.CB_L * uniq.shape[0])).reshape(uniq.shape[0], cb.CB_L, cb.PKS_IN)[pattern]
        else:
            stage1 = l2m.cb_rotate_batch(self.ring, uniq)[pattern]
        r["trgsw"] = cb.trgsw_from_stage1(self.pks_key, stage1).reshape(D, TRGSW)
        # the CMUX follows call 1 of the chain, whose row g holds the selector of input g + 1
        r["res"] = pmap(lambda d: prc.cmux(self.keys.L, r["trgsw"][(d + 1) % D], r["c1"][d], r["c0"][d]), D)
        return r

    def need_pks(self):
        if self.pks_key is None:
            self.pks_key = np.random.default_rng(2024).integers(0, 2**32, size=cb.PKS_KEY_WORDS, dtype=np.uint32)
            self.api.cb_initialize(self.pks_key)
        return self.pks_key

    def ref_pks(self, v):
        t2 = np.random.default_rng(8700 + v).integers(0, 2**64, size=(D, cb.PKS_IN), dtype=np.uint64)
        t2[0] = 0
        t2[1] = np.uint64(2**64 - 1)
        return dict(t2=t2, out=cb.private_keyswitch_batch(self.pks_key, t2).reshape(D, 2 * TR))

    # -- a compiled set with a two-limb key
    def need_ps(self):
        if self.ps is None:
            K = ol.Keys(ol.load_set("cggi16"), seed=5)
            idx = self.api.ps_index("cggi16")
            self.api.ps_initialize(idx, K.bk, K.ksk)
            self.ps = (idx, K, self.api.ps_params(idx))
        return self.ps

    def ref_ps(self, v):
        idx, K, p = self.ps
        s = 8900 + 100 * v
        w0, w1, tr = K.words[0], K.words[1], (K.k + 1) * K.N
        trgsw = (K.k + 1) * ol.set_params(K.L)[1]["l"] * tr
        r = dict(a=rnd(s, D, w0), b=rnd(s + 1, D, w0), l1a=rnd(s + 2, D, w1), l1b=rnd(s + 3, D, w1), tg=rnd(s + 4, D, trgsw),
                 c1=rnd(s + 5, D, tr), c0=rnd(s + 6, D, tr))
        r["ops"] = np.array([OPS["NAND"] if (d + v) % 2 else OPS["XNOR"] for d in range(D)], np.int32)
        r["x1"] = K.gate_batch(r["ops"], 0, r["a"], r["b"])
        r["x2"] = K.gate_batch(r["ops"], 0, r["x1"], r["b"])
        r["y"] = K.gate_batch(r["ops"], 1, r["l1a"], r["l1b"])

        def cmux(d):
            w = np.zeros(tr, U32)
            K.L.orc_cmux(w, np.ascontiguousarray(r["tg"][d]), np.ascontiguousarray(r["c1"][d]), np.ascontiguousarray(r["c0"][d]))
            return w
        r["res"] = pmap(cmux, D)
        return r


@pytest.fixture(scope="module")
def world(engine, keys):
    """a freshly initialised engine with the module's definitions; the session's state again afterwards"""
    def reinit():
        engine.CleanUp()
        engine.SetGPUNum(1)
        engine.Initialize(keys.bk, keys.ksk)
    reinit()
    assert fp.csrc_constant("kKsMmRows", ("kernels_ks2.hip.h",)) == sc.KS_MM_ROWS
    w = World(engine, keys)
    yield w
    w.destroy_streams()
    reinit()


@pytest.fixture
def streams(world):
    """created streams for one test, destroyed behind it"""
    made = []

    def make(count=1):
        made.extend(world.stream() for _ in range(count))
        return [s.st() for s in made[-count:]]
    yield make
    for s in made:
        if s.st():
            s.Destroy()
        world.streams.remove(s)


# ---------------------------------------------------------------------------------------------------------------------------------
# the chains
# ---------------------------------------------------------------------------------------------------------------------------------
def gate_chain(world, st, v, counts=sc.GATE_COUNTS, ks_counts=sc.KS_COUNTS, label="gate chain"):
    """gate_batch (NAND / XOR) -> gate_batch (a user gate and MUX on the results) -> bootstrap_batch, refresh_batch ->
    sample_extract_keyswitch_batch -> gate_batch at level 1 -> keyswitch_batch four times -> gate_batch on the key switches' words.
    counts: the gate path's 8 -> 1024 -> 8 -> 4096 -> 9."""
    api, r = world.api, world.ref("gate", v)
    c1, c2, c3, c4, c5 = counts
    assert max(ks_counts) <= c4 and c5 <= ks_counts[-1]
    L = Lane(world.eng, f"{label} {v}", st)
    L.inp("a", pos.tile(r["a"], max(c1, c5)))
    L.inp("b", pos.tile(r["b"], max(c1, c2)))
    L.inp("c", pos.tile(r["c"], c2))
    L.inp("T", pos.tile(r["T"], c3))
    L.inp("l1a", pos.tile(r["l1a"], c4))
    L.inp("l1b", pos.tile(r["l1b"], c4))
    L.out("x1", r["x1"], c1, rows=c2)
    L.out("x2", r["x2"], c2, rows=c3)
    L.out("x3", r["x3"], c3)
    L.out("r3", r["r3"], c3)
    L.out("x4", r["x4"], c3)
    L.out("y5", r["y5"], c4)
    for k, c in enumerate(ks_counts):
        L.out(f"x6_{k}", r["x6"], c)
    L.out("x7", r["x7"], c5)
    ops1, ops2, ops5 = (pos.tile(r[k], c) for k, c in (("ops1", c1), ("ops2", c2), ("ops5", c4)))
    L.call("gate_batch level 0", lambda: api.gate_batch(ops1, 0, L.v("x1"), L.v("a"), L.v("b"), count=c1, stream=st))
    L.call("gate_batch user gate + MUX", lambda: api.gate_batch(ops2, 0, L.v("x2"), L.v("x1"), L.v("b"), L.v("c"), count=c2, stream=st))
    L.call("bootstrap_batch", lambda: api.bootstrap_batch(L.v("x3"), L.v("x2"), c3, stream=st))
    L.call("refresh_batch", lambda: api.refresh_batch(L.v("T"), L.v("r3"), c3, stream=st))
    L.call("sample_extract_keyswitch_batch", lambda: api.sample_extract_keyswitch_batch(L.v("r3"), L.v("x4"), c3, stream=st))
    L.call("gate_batch level 1", lambda: api.gate_batch(ops5, 1, L.v("y5"), L.v("l1a"), L.v("l1b"), count=c4, stream=st))
    for k, c in enumerate(ks_counts):
        L.call(f"keyswitch_batch {c}", lambda k=k, c=c: api.keyswitch_batch(L.v("y5"), L.v(f"x6_{k}"), c, stream=st))
    last = len(ks_counts) - 1
    L.call("gate_batch on the key switches", lambda: api.gate_batch(OPS["NAND"], 0, L.v("x7"), L.v(f"x6_{last}"), L.v("a"), count=c5, stream=st))
    return L


def short_gate_chain(world, st, v, counts, label="short gate chain"):
    """the first three calls of the gate chain"""
    api, r = world.api, world.ref("gate", v)
    c1, c2, c3 = counts
    L = Lane(world.eng, f"{label} {v}", st)
    L.inp("a", pos.tile(r["a"], c1))
    L.inp("b", pos.tile(r["b"], max(c1, c2)))
    L.inp("c", pos.tile(r["c"], c2))
    L.out("x1", r["x1"], c1, rows=c2)
    L.out("x2", r["x2"], c2, rows=c3)
    L.out("x3", r["x3"], c3)
    ops1, ops2 = pos.tile(r["ops1"], c1), pos.tile(r["ops2"], c2)
    L.call("gate_batch level 0", lambda: api.gate_batch(ops1, 0, L.v("x1"), L.v("a"), L.v("b"), count=c1, stream=st))
    L.call("gate_batch user gate + MUX", lambda: api.gate_batch(ops2, 0, L.v("x2"), L.v("x1"), L.v("b"), L.v("c"), count=c2, stream=st))
    L.call("bootstrap_batch", lambda: api.bootstrap_batch(L.v("x3"), L.v("x2"), c3, stream=st))
    return L


# counts of the TRLWE chain: TRGSW2NTT, CMUX, rotating CMUX | rotation | extraction + key switch | packed outputs | Spread | lookups.
# The workspace holds only descriptors up to the extraction (a few KiB: the first block of 1 MiB and a little serves them all); 300
# extractions need 300 * 1025 * 4 + (4 * 300 + 8) * 40 + 16384 = 1 294 704 bytes (trlwe_batch) > that block and leave one of 2 666 956;
# the pack, the Spread's neighbours and 9 lookups reuse it shrunk; 1031 lookups of two outputs (1031 (2 (4100 + 40) + 48) + 8192 =
# 8 594 360, the short form's 400: 3 339 392) regrow it while the calls before them may still run.
TRLWE_COUNTS = (40, 300, 300, 8, 9, 1031)
TRLWE_SHORT = (12, 40, 300, 8, 9, 400)


def trlwe_chain(world, st, v, counts=TRLWE_COUNTS, label="TRLWE chain"):
    api, r = world.api, world.ref("trlwe", v)
    cn, crot, cse, cpk, csp, clu = counts
    L = Lane(world.eng, f"{label} {v}", st)
    L.inp("tg", pos.tile(r["tg"], cn))
    L.inp("c1", pos.tile(r["c1"], cn))
    L.inp("c0", pos.tile(r["c0"], cn))
    L.inp("addr", pos.tile(r["addr"], clu))
    L.out("ntt", np.zeros((D, 2 * TRGSW), U32), cn)        # doubles; checked through the products, never read past its live rows
    L.checks.pop()
    L.out("r3", r["r3"], cn, rows=crot)                    # CMUX writes it, the rotating CMUX rewrites it in place
    L.out("r4", r["r4"], crot, rows=cse)
    L.out("x5", r["x5"], cse, rows=2 * cpk)
    L.out("p6", r["p6"], cpk, rows=csp)
    L.out("s7", r["s7"], csp, rows=clu)
    L.out("o8", r["o8"], clu)
    e3, e4, idx5 = pos.tile(r["e3"], cn), pos.tile(r["e4"], crot), pos.tile(r["idx5"], cse)
    m = np.arange(2 * cpk)
    dst6, pos6 = (m // 2).astype(np.int32), np.ascontiguousarray(r["pos6"][m % (2 * D)])
    L.call("trgsw_to_ntt_batch", lambda: api.trgsw_to_ntt_batch(L.v("tg"), L.v("ntt"), cn, stream=st))
    L.call("cmux_batch", lambda: api.cmux_batch(L.v("ntt"), L.v("c1"), L.v("c0"), L.v("r3"), cn, stream=st))
    L.call("cmux_rotate_batch in place", lambda: api.cmux_rotate_batch(L.v("ntt"), e3, L.v("r3"), L.v("r3"), cn, stream=st))
    L.call("trlwe_rotate_batch", lambda: api.trlwe_rotate_batch(L.v("r3"), e4, L.v("r4"), crot, stream=st))
    L.call("sample_extract_index_keyswitch_batch", lambda: api.sample_extract_index_keyswitch_batch(L.v("r4"), idx5, L.v("x5"), cse, stream=st))
    L.call("pack_batch", lambda: api.pack_batch(L.v("x5"), dst6, pos6, L.v("p6"), 2 * cpk, cpk, stream=st))
    L.call("trlwe_spread_batch", lambda: api.trlwe_spread_batch(L.v("p6"), L.v("s7"), csp, world.STRIDE, world.REPS, stream=st))
    L.call("lut_lookup_batch nout 2", lambda: api.lut_lookup_batch(L.v("addr"), L.v("s7"), L.v("o8"), clu, clu, nout=2, stream=st))
    return L


# sets of the linear chain: sets * rows = 3 -> 66 -> 3 -> 264 gates behind linear_gate_batch, so that g_linear_tmp (the exact size) and,
# under the matrix key switch, ks_digits (1, 2, 1, 5 tiles) regrow twice and are reused shrunk in between; the workspace regrows at
# 88 sets (need(264) = 1 820 608 > the first block)
LINEAR_SETS = (1, 22, 1, 88)


def linear_chain(world, st, v, sets=LINEAR_SETS, label="linear chain"):
    """linear_batch -> linear_gate_batch on its sums, four sizes -> gate_batch on the activations"""
    api, r = world.api, world.ref("linear", v)
    top = max(sets)
    L = Lane(world.eng, f"{label} {v}", st)
    L.inp("x", pos.tile(r["x"], top))
    L.inp("bb", pos.tile(r["bb"], sets[-1]))
    L.out("y1", r["y1"], top)
    for k, s in enumerate(sets):
        L.out(f"y2_{k}", r["y2"], s)
    L.out("g3", r["g3"], sets[-1])
    L.call("linear_batch", lambda: api.linear_batch(world.layer1, 0, L.v("y1"), L.v("x"), top, stream=st))
    for k, s in enumerate(sets):
        L.call(f"linear_gate_batch {s} sets",
               lambda k=k, s=s: api.linear_gate_batch(world.layer2, world.user1["op"], 0, L.v(f"y2_{k}"), L.v("y1"), s, stream=st))
    last = len(sets) - 1
    L.call("gate_batch on the activations",
           lambda: api.gate_batch(OPS["NAND"], 0, L.v("g3"), L.v(f"y2_{last}"), L.v("bb"), count=3 * sets[-1], stream=st))
    return L


def ks_chain(world, st, v, counts=sc.KS_COUNTS, label="key switches"):
    api, r = world.api, world.ref("ks", v)
    L = Lane(world.eng, f"{label} {v}", st)
    L.inp("y", pos.tile(r["y"], max(counts)))
    for k, c in enumerate(counts):
        L.out(f"x{k}", r["x"], c)
        L.call(f"keyswitch_batch {c}", lambda k=k, c=c: api.keyswitch_batch(L.v("y"), L.v(f"x{k}"), c, stream=st))
    return L


def ring_chain(world, st, v, counts=(8, 300, 9), label="N = 2048 ring"):
    api, r = world.api, world.ref("ring", v)
    c1, c2, c3 = counts
    L = Lane(world.eng, f"{label} {v}", st)
    L.inp("a", pos.tile(r["a"], c1))
    L.inp("b", pos.tile(r["b"], max(counts)))
    L.out("x1", r["x1"], c1, rows=c2)
    L.out("x2", r["x2"], c2)
    L.out("x2b", r["x2"], c3)
    ops1, ops2 = pos.tile(r["ops1"], c1), pos.tile(r["ops2"], c2)
    L.call("lvl2_gate_batch", lambda: api.lvl2_gate_batch(ops1, L.v("x1"), L.v("a"), L.v("b"), count=c1, stream=st))
    L.call("lvl2_gate_batch on the results", lambda: api.lvl2_gate_batch(ops2, L.v("x2"), L.v("x1"), L.v("b"), count=c2, stream=st))
    L.call("lvl2_gate_batch, fewer", lambda: api.lvl2_gate_batch(ops2, L.v("x2b"), L.v("x1"), L.v("b"), count=c3, stream=st))
    return L


def pks_chain(world, st, v, counts=(1, 65, 3), label="private key switches"):
    api, r = world.api, world.ref("pks", v)
    L = Lane(world.eng, f"{label} {v}", st)
    L.inp("t2", pos.tile(r["t2"], max(counts)))
    for k, c in enumerate(counts):
        L.out(f"out{k}", r["out"], c)
        L.call(f"private_keyswitch_batch {c}", lambda k=k, c=c: api.private_keyswitch_batch(L.v("t2"), L.v(f"out{k}"), c, stream=st))
    return L


def extract_chain(world, st, v, counts=(8, 65, 9), label="lvl2 user extraction -> private key switch"):
    api, r, u = world.api, world.ref("extract", v), world.user_ring
    c1, c2, c3 = counts
    L = Lane(world.eng, f"{label} {v}", st)
    L.inp("a", pos.tile(r["a"], max(c1, c3)))
    L.inp("b", pos.tile(r["b"], max(c1, c3)))
    L.out("t2", r["t2"], c1, rows=c2)
    L.out("out", r["out"], c2)
    L.out("t2b", r["t2"], c3)
    L.call("lvl2_user_extract_batch", lambda: api.lvl2_user_extract_batch(u["op"], L.v("a"), L.v("t2"), c1, in1=L.v("b"), stream=st))
    L.call("private_keyswitch_batch", lambda: api.private_keyswitch_batch(L.v("t2"), L.v("out"), c2, stream=st))
    L.call("lvl2_user_extract_batch, again", lambda: api.lvl2_user_extract_batch(u["op"], L.v("a"), L.v("t2b"), c3, in1=L.v("b"), stream=st))
    return L


def cb_chain(world, st, rotations, counts=(1, 40, 2), label="circuit bootstraps"):
    """circuit_bootstrap_batch three times (one circuit bootstrap keeps 3 * 2049 * 8 = 49 176 bytes of lvl2 words in the workspace and its
    rotations' scratch on top: 40 of them outgrow the first block of 1 MiB and a little, 2 reuse it shrunk), the middle one followed by a
    CMUX with the NTT-domain selectors it made"""
    api, r = world.api, world.ref("cb", rotations)
    c1, c2, c3 = counts
    L = Lane(world.eng, f"{label}, cb_rotations {rotations}", st)
    L.inp("x", pos.tile(r["x"], max(counts) + len(counts)))
    L.inp("c1", pos.tile(r["c1"], c2))
    L.inp("c0", pos.tile(r["c0"], c2))
    for k, c in enumerate(counts):
        L.out(f"trgsw{k}", np.roll(r["trgsw"], -k, axis=0), c)       # call k reads the inputs from row k on
    L.out("ntt", np.zeros((D, 2 * TRGSW), U32), c2)
    L.checks.pop()
    L.out("res", r["res"], c2)
    L.call("circuit_bootstrap_batch", lambda: api.circuit_bootstrap_batch(L.v("x", 0), c1, trgsw=L.v("trgsw0"), stream=st))
    L.call("circuit_bootstrap_batch, torus and NTT", lambda: api.circuit_bootstrap_batch(L.v("x", 1), c2, trgsw=L.v("trgsw1"), trgsw_ntt=L.v("ntt"), stream=st))
    L.call("cmux_batch with the new selectors", lambda: api.cmux_batch(L.v("ntt"), L.v("c1"), L.v("c0"), L.v("res"), c2, stream=st))
    L.call("circuit_bootstrap_batch, fewer", lambda: api.circuit_bootstrap_batch(L.v("x", 2), c3, trgsw=L.v("trgsw2"), stream=st))
    return L


def pack_chain(world, st, v, counts=(1, 65, 3), label="packs"):
    """pack_batch alone, two inputs per output, from the expected extraction words of the TRLWE chain"""
    api, r = world.api, world.ref("trlwe", v)
    L = Lane(world.eng, f"{label} {v}", st)
    L.inp("x5", pos.tile(r["x5"], 2 * max(counts)))
    keep = []
    for k, c in enumerate(counts):
        m = np.arange(2 * c)
        dst, p = (m // 2).astype(np.int32), np.ascontiguousarray(r["pos6"][m % (2 * D)])
        keep.append((dst, p))
        L.out(f"p{k}", r["p6"], c)
        L.call(f"pack_batch {c}", lambda k=k, c=c, dst=dst, p=p: api.pack_batch(L.v("x5"), dst, p, L.v(f"p{k}"), 2 * c, c, stream=st))
    return L


def lookup_chain(world, st, v, counts=(9, 260, 3), label="lookups"):
    api, r = world.api, world.ref("trlwe", v)
    L = Lane(world.eng, f"{label} {v}", st)
    L.inp("addr", pos.tile(r["addr"], max(counts)))
    L.inp("s7", pos.tile(r["s7"], max(counts)))
    for k, c in enumerate(counts):
        L.out(f"o{k}", r["o8"], c)
        L.call(f"lut_lookup_batch {c}", lambda k=k, c=c: api.lut_lookup_batch(L.v("addr"), L.v("s7"), L.v(f"o{k}"), c, c, nout=2, stream=st))
    return L


def spread_chain(world, st, v, counts=(9, 260, 3), label="Spreads"):
    api, r = world.api, world.ref("trlwe", v)
    L = Lane(world.eng, f"{label} {v}", st)
    L.inp("p6", pos.tile(r["p6"], max(counts)))
    for k, c in enumerate(counts):
        L.out(f"s{k}", r["s7"], c)
        L.call(f"trlwe_spread_batch {c}", lambda k=k, c=c: api.trlwe_spread_batch(L.v("p6"), L.v(f"s{k}"), c, world.STRIDE, world.REPS, stream=st))
    return L


def ps_chain(world, st, v, counts=(8, 300, 9), label="cggi16"):
    """ps_gate_batch_level at both levels, ps_trgsw_to_ntt_batch -> ps_cmux_batch"""
    api, r = world.api, world.ref("ps", v)
    idx, K, p = world.ps
    c1, c2, c3 = counts
    L = Lane(world.eng, f"{label} {v}", st)
    L.inp("a", pos.tile(r["a"], c1))
    L.inp("b", pos.tile(r["b"], max(c1, c2)))
    L.inp("l1a", pos.tile(r["l1a"], c3))
    L.inp("l1b", pos.tile(r["l1b"], c3))
    for k in ("tg", "c1", "c0"):
        L.inp(k, pos.tile(r[k], c3))
    L.out("x1", r["x1"], c1, rows=c2)
    L.out("x2", r["x2"], c2)
    L.out("y", r["y"], c3)
    L.out("ntt", np.zeros((D, r["tg"].shape[1] * 2 * p.key_limbs), U32), c3)
    L.checks.pop()
    L.out("res", r["res"], c3)
    ops1, ops2, ops3 = (pos.tile(r["ops"], c) for c in counts)
    L.call("ps_gate_batch level 0", lambda: api.ps_gate_batch(idx, ops1, L.v("x1"), L.v("a"), L.v("b"), count=c1, stream=st, level=0))
    L.call("ps_gate_batch level 0 on the results", lambda: api.ps_gate_batch(idx, ops2, L.v("x2"), L.v("x1"), L.v("b"), count=c2, stream=st, level=0))
    L.call("ps_gate_batch level 1", lambda: api.ps_gate_batch(idx, ops3, L.v("y"), L.v("l1a"), L.v("l1b"), count=c3, stream=st, level=1))
    L.call("ps_trgsw_to_ntt_batch", lambda: api.ps_trgsw_to_ntt_batch(idx, L.v("tg"), L.v("ntt"), c3, stream=st))
    L.call("ps_cmux_batch", lambda: api.ps_cmux_batch(idx, L.v("ntt"), L.v("c1"), L.v("c0"), L.v("res"), c3, stream=st))
    return L


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. chains on one stream without a synchronise
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks_mm", [1, 0], ids=["matrix-keyswitch", "rule-keyswitch"])
def test_gate_chain_on_one_stream(world, streams, ks_mm):
    """8 -> 1024 -> 8 -> 4096 -> 9 gates and 1 -> 65 -> 1 -> 260 key switches: the workspace regrows twice and is reused shrunk twice
    (tests/test_stream_contract.py), under "ks_mm_threshold" 1 the digit words of the matrix key switch as well"""
    st, = streams()
    with pos.options(world.api, dict(ks_mm_threshold=ks_mm)):
        run_lanes([gate_chain(world, st, 0)])


def test_trlwe_chain_on_one_stream(world, streams):
    st, = streams()
    run_lanes([trlwe_chain(world, st, 0)])


@pytest.mark.parametrize("ks_mm", [1, 0], ids=["matrix-keyswitch", "rule-keyswitch"])
def test_linear_chain_on_one_stream(world, streams, ks_mm):
    st, = streams()
    with pos.options(world.api, dict(ks_mm_threshold=ks_mm)):
        run_lanes([linear_chain(world, st, 0)])


def test_ring_chain_on_one_stream(world, streams, oracle):
    world.need_ring(oracle)
    st, = streams()
    run_lanes([ring_chain(world, st, 0)])


def test_private_keyswitch_chain_on_one_stream(world, streams):
    world.need_pks()
    st, = streams()
    run_lanes([pks_chain(world, st, 0)])


def test_extraction_into_private_keyswitch_on_one_stream(world, streams, oracle):
    world.need_ring_gate(oracle)
    world.need_pks()
    st, = streams()
    run_lanes([extract_chain(world, st, 0)])


@pytest.mark.parametrize("rotations", [3, 1])
def test_circuit_bootstrap_chain_on_one_stream(world, streams, oracle, rotations):
    world.need_ring(oracle)
    world.need_pks()
    st, = streams()
    with pos.options(world.api, dict(cb_rotations=rotations)):
        run_lanes([cb_chain(world, st, rotations)])


def test_paramset_chain_on_one_stream(world, streams):
    world.need_ps()
    st, = streams()
    run_lanes([ps_chain(world, st, 0)])


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. host argument arrays belong to the caller again on return
# ---------------------------------------------------------------------------------------------------------------------------------
COUNT2 = 300


class Occupied:
    """a stream kept busy by 1024 bootstraps (about 10 ms): what is issued behind them cannot have run when its call returns"""

    def __init__(self, world, st):
        self.world, self.st = world, st
        self.din = world.api.DeviceBuffer(1024 * W0).upload(rnd(9001, 1024 * W0))
        self.dout = world.api.DeviceBuffer(1024 * W0)

    def occupy(self):
        device_call(self.world.eng, lambda: self.world.api.bootstrap_batch(self.dout, self.din, 1024, stream=self.st), "the occupying bootstraps")

    def close(self):
        self.din.free()
        self.dout.free()


def overwritten_after_return(world, st, lane, arrays, others, expected_other, pointers=None):
    """lane: calls whose host arrays are `arrays`; behind the occupying launch they are issued, every array is overwritten in place with
    the array of `others`, and the words must be the checker's for the ORIGINAL arrays -- which differ in every row from the checker's
    words for the overwriting ones (expected_other: [(want, want_other)]), so a late read cannot pass.  pointers: a function of the built
    lane that returns more (arrays, others) -- lists of device pointers exist only once the arena does."""
    for want, want_other in expected_other:
        assert sc.differs_in_every_row(want, want_other), "the overwriting values give the same words in some row: the test could not fail"
    occ = Occupied(world, st)
    try:
        lane.build()
        if pointers:
            more = pointers(lane)
            arrays, others = list(arrays) + list(more[0]), list(others) + list(more[1])
        for a, o in zip(arrays, others):
            assert a.dtype == o.dtype and a.shape == o.shape and a.flags.c_contiguous and not np.array_equal(a, o)
        occ.occupy()
        for i in range(len(lane.calls)):
            lane.issue(i)
        for a, o in zip(arrays, others):
            a[...] = o
        lane.sync()
        bad = lane.failures()
    finally:
        lane.close()
        occ.close()
    assert not bad, "\n".join(bad)


def pointer_lists(lane, table, pairs):
    """table[name] = the device pointers of the rows of operand `name` (uint64, what the list entry points take) for every (name, decoy,
    rows) of `pairs`; returns (those arrays, the same rows of the decoy operands)"""
    arrays, others = [], []
    for name, decoy, rows in pairs:
        offs = np.arange(rows, dtype=np.uint64) * np.uint64(4 * W0)
        table[name] = np.uint64(lane.arena.ptr(name)) + offs
        arrays.append(table[name])
        others.append(np.uint64(lane.arena.ptr(decoy)) + offs)
    return arrays, others


def test_host_ops_of_gate_batch(world, streams):
    st, = streams()
    api, K, r = world.api, world.keys, world.ref("gate", 0)
    ops = pos.tile(r["ops1"], COUNT2)
    other = sc.other_ops(ops)
    want_other = K.gate_batch(sc.other_ops(r["ops1"]), 0, r["a"], r["b"])
    L = Lane(world.eng, "gate_batch, ops overwritten", st)
    L.inp("a", pos.tile(r["a"], COUNT2))
    L.inp("b", pos.tile(r["b"], COUNT2))
    L.out("x1", r["x1"], COUNT2)
    L.call("gate_batch", lambda: api.gate_batch(ops, 0, L.v("x1"), L.v("a"), L.v("b"), count=COUNT2, stream=st))
    overwritten_after_return(world, st, L, [ops], [other], [(r["x1"], want_other)])


def test_host_ops_and_pointer_lists_of_gate_list(world, streams):
    """ops and the pointer lists: the overwriting pointers name decoy buffers of the right size -- other ciphertexts as operands, a decoy
    output that must still hold its poison afterwards (it is an input of the arena: a store to it is a finding)"""
    st, = streams()
    K, r, lib = world.keys, world.ref("gate", 0), world.eng.lib
    a2, b2 = np.roll(r["a"], 1, axis=0), np.roll(r["b"], 3, axis=0)
    ops = pos.tile(r["ops1"], COUNT2)
    want_other = K.gate_batch(sc.other_ops(r["ops1"]), 0, a2, b2)
    L = Lane(world.eng, "gate_list, ops and pointers overwritten", st)
    for name, rows in (("a", r["a"]), ("b", r["b"]), ("a2", a2), ("b2", b2)):
        L.inp(name, pos.tile(rows, COUNT2))
    L.inp("decoy", pos.poison((COUNT2, W0)))
    L.out("x1", r["x1"], COUNT2)
    p = {}
    L.call("gate_list", lambda: world.eng.check(lib.cufhe_amd_gate_list(0, st, 0, COUNT2, ops.ctypes.data, p["x1"].ctypes.data,
                                                                        p["a"].ctypes.data, p["b"].ctypes.data, None)))
    overwritten_after_return(world, st, L, [ops], [sc.other_ops(ops)], [(r["x1"], want_other)],
                             pointers=lambda lane: pointer_lists(lane, p, [("x1", "decoy", COUNT2), ("a", "a2", COUNT2), ("b", "b2", COUNT2)]))


def test_host_pointer_lists_of_linear_list(world, streams):
    st, = streams()
    r, lib = world.ref("linear", 0), world.eng.lib
    sets = 40
    x2 = np.roll(r["x"], 2, axis=0)
    want_other = lin.linear(world.W1m, world.b1, x2)
    L = Lane(world.eng, "linear_list, pointers overwritten", st)
    L.inp("x", pos.tile(r["x"], sets))
    L.inp("x2", pos.tile(x2, sets))
    L.inp("decoy", pos.poison((sets, 3 * W0)))
    L.out("y1", r["y1"], sets)
    p = {}
    L.call("linear_list", lambda: world.eng.check(lib.cufhe_amd_linear_list(0, st, world.layer1.id, 0, sets, p["x"].ctypes.data, p["y1"].ctypes.data)))
    overwritten_after_return(world, st, L, [], [], [(r["y1"], want_other)],
                             pointers=lambda lane: pointer_lists(lane, p, [("y1", "decoy", 3 * sets), ("x", "x2", 2 * sets)]))


def test_host_exponents_of_the_rotations(world, streams):
    """exps of trlwe_rotate_batch and of cmux_rotate_batch, in one lane"""
    st, = streams()
    api, K, r = world.api, world.keys, world.ref("trlwe", 0)
    e4, e3 = pos.tile(r["e4"], COUNT2), pos.tile(r["e3"], COUNT2)
    o4, o3 = sc.other_in_range(e4, 2 * N, 1031), sc.other_in_range(e3, 2 * N, 517)
    rot = np.stack([prc.rotate(r["c1"][d], int(r["e4"][d])) for d in range(D)])
    rot_other = np.stack([prc.rotate(r["c1"][d], int((r["e4"][d] + 1031) % (2 * N))) for d in range(D)])
    cr = pmap(lambda d: prc.cmux_rotate(K.L, r["tg"][0], r["c0"][d], int(r["e3"][d])), D)
    cr_other = pmap(lambda d: prc.cmux_rotate(K.L, r["tg"][0], r["c0"][d], int((r["e3"][d] + 517) % (2 * N))), D)
    L = Lane(world.eng, "rotations, exponents overwritten", st)
    L.inp("tg", r["tg"][:1])
    L.inp("c1", pos.tile(r["c1"], COUNT2))
    L.inp("c0", pos.tile(r["c0"], COUNT2))
    L.out("ntt", np.zeros((D, 2 * TRGSW), U32), 1)
    L.checks.pop()
    L.out("rot", rot, COUNT2)
    L.out("cr", cr, COUNT2)
    L.call("trgsw_to_ntt_batch", lambda: api.trgsw_to_ntt_batch(L.v("tg"), L.v("ntt"), 1, stream=st))
    L.call("trlwe_rotate_batch", lambda: api.trlwe_rotate_batch(L.v("c1"), e4, L.v("rot"), COUNT2, stream=st))
    L.call("cmux_rotate_batch", lambda: api.cmux_rotate_batch(L.v("ntt"), e3, L.v("c0"), L.v("cr"), COUNT2, stream=st))
    overwritten_after_return(world, st, L, [e4, e3], [o4, o3], [(rot, rot_other), (cr, cr_other)])


def test_host_indices_of_the_extractions(world, streams):
    """src / idx of sample_extract_index_batch and of sample_extract_index_keyswitch_batch"""
    st, = streams()
    api, K, r = world.api, world.keys, world.ref("trlwe", 0)
    g = np.arange(COUNT2)
    src = ((g + 3 * (g % D)) % COUNT2).astype(np.int32)                     # row g reads TRLWE src[g], which carries input (g + 3 (g % D)) % COUNT2 % D
    idx = pos.tile(r["idx5"], COUNT2)
    src_o, idx_o = sc.other_in_range(src, COUNT2, 1), sc.other_in_range(idx, N, 389)
    trl = pos.tile(r["c1"], COUNT2)
    # COUNT2 = 300 = 6 mod 7: the source input of row g is not a function of g % D alone, so the reference is computed per distinct
    # (source input, index) pair and gathered per row
    def words(src_, idx_, ks):
        pairs = sorted({(int(s) % D, int(j)) for s, j in zip(src_, idx_)})
        table = dict(zip(pairs, pmap(lambda i: (prc.extract_keyswitch(K, r["c1"][pairs[i][0]], pairs[i][1]) if ks
                                               else prc.extract_formula(r["c1"][pairs[i][0]], pairs[i][1])), len(pairs))))
        return np.stack([table[int(s) % D, int(j)] for s, j in zip(src_, idx_)])
    want1, other1 = words(src, idx, False), words(src_o, idx_o, False)
    want0, other0 = words(src, idx, True), words(src_o, idx_o, True)
    assert sc.differs_in_every_row(want1, other1) and sc.differs_in_every_row(want0, other0)
    src2, idx2 = src.copy(), idx.copy()
    d_trl = api.DeviceBuffer(trl.size).upload(trl)
    d1 = api.DeviceBuffer(COUNT2 * W1).upload(pos.poison(COUNT2 * W1))
    d0 = api.DeviceBuffer(COUNT2 * W0).upload(pos.poison(COUNT2 * W0))
    occ = Occupied(world, st)
    try:
        occ.occupy()
        device_call(world.eng, lambda: api.sample_extract_index_batch(d_trl, idx, d1, COUNT2, src=src, stream=st), "sample_extract_index_batch")
        src[...] = src_o
        idx[...] = idx_o
        device_call(world.eng, lambda: api.sample_extract_index_keyswitch_batch(d_trl, idx2, d0, COUNT2, src=src2, stream=st),
                    "sample_extract_index_keyswitch_batch")
        src2[...] = src_o
        idx2[...] = idx_o
        synchronize(world.eng, st, "indexed extractions")
        got1, got0 = d1.download().reshape(COUNT2, W1), d0.download().reshape(COUNT2, W0)
    finally:
        for b in (d_trl, d1, d0):
            b.free()
        occ.close()
    for got, want, other, name in ((got1, want1, other1, "sample_extract_index_batch"), (got0, want0, other0, "sample_extract_index_keyswitch_batch")):
        bad = np.flatnonzero((got != want).any(axis=1))
        late = np.flatnonzero((got == other).all(axis=1))
        assert bad.size == 0, f"{name}: rows {bad[:10].tolist()} differ from the checker; {late.size} rows hold the words of the overwriting src / idx"


def test_host_src_of_the_lookups(world, streams):
    """src of lut_rotate_batch (3 steps) and of lut_lookup_batch: seven tables, row g reads table src[g]"""
    st, = streams()
    api, K, r = world.api, world.keys, world.ref("trlwe", 0)
    count = 70
    g = np.arange(count)
    src = ((3 * g + 1) % D).astype(np.int32)
    src_o = sc.other_in_range(src, D, 2)
    addr = pos.tile(r["addr"], count)

    def words(src_, lookup):
        pairs = sorted({(int(q) % D, int(s)) for q, s in zip(g, src_)})
        fn = (lambda i: lc.lut_lookup(K, r["addr"][pairs[i][0]], r["s7"][pairs[i][1]], 1)[0]) if lookup else \
             (lambda i: lc.lut_rotate(K, r["addr"][pairs[i][0]], r["s7"][pairs[i][1]], 0, 3))
        table = dict(zip(pairs, pmap(fn, len(pairs))))
        return np.stack([table[int(q) % D, int(s)] for q, s in zip(g, src_)])
    want_r, other_r = words(src, False), words(src_o, False)
    want_l, other_l = words(src, True), words(src_o, True)
    assert sc.differs_in_every_row(want_r, other_r) and sc.differs_in_every_row(want_l, other_l)
    src2 = src.copy()
    d_addr = api.DeviceBuffer(addr.size).upload(addr)
    d_tab = api.DeviceBuffer(D * TR).upload(r["s7"])
    d_acc = api.DeviceBuffer(count * TR).upload(pos.poison(count * TR))
    d_out = api.DeviceBuffer(count * W0).upload(pos.poison(count * W0))
    occ = Occupied(world, st)
    try:
        occ.occupy()
        device_call(world.eng, lambda: api.lut_rotate_batch(d_addr, d_tab, d_acc, count, D, src=src, nout=1, steps=3, stream=st), "lut_rotate_batch")
        src[...] = src_o
        device_call(world.eng, lambda: api.lut_lookup_batch(d_addr, d_tab, d_out, count, D, src=src2, nout=1, stream=st), "lut_lookup_batch")
        src2[...] = src_o
        synchronize(world.eng, st, "lookups")
        got_r, got_l = d_acc.download().reshape(count, TR), d_out.download().reshape(count, W0)
    finally:
        for b in (d_addr, d_tab, d_acc, d_out):
            b.free()
        occ.close()
    for got, want, name in ((got_r, want_r, "lut_rotate_batch"), (got_l, want_l, "lut_lookup_batch")):
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f"{name}: rows {bad[:10].tolist()} differ from the checker"


def test_host_dst_and_pos_of_pack_batch(world, streams):
    st, = streams()
    api, r = world.api, world.ref("trlwe", 0)
    cout = 150
    m = np.arange(2 * cout)
    dst, p = (m // 2).astype(np.int32), np.ascontiguousarray(r["pos6"][m % (2 * D)])
    # the other values: every input moves to the NEXT output (dst + 1 mod cout) and to another position
    dst_o, p_o = sc.other_in_range(dst, cout, 1), sc.other_in_range(p, N, 389)
    x = pos.tile(r["x5"], 2 * cout)
    # the checker on the overwriting arrays, all outputs (the wrap of the last inputs to output 0 included), against all expected rows
    assert sc.differs_in_every_row(pos.tile(r["p6"], cout), pk.pack_batch(world.pack_key, x, dst_o, p_o, cout))
    L = Lane(world.eng, "pack_batch, dst and pos overwritten", st)
    L.inp("x5", x)
    L.out("p6", r["p6"], cout)
    L.call("pack_batch", lambda: api.pack_batch(L.v("x5"), dst, p, L.v("p6"), 2 * cout, cout, stream=st))
    overwritten_after_return(world, st, L, [dst, p], [dst_o, p_o], [])


def test_host_ops_of_the_ring_and_of_a_set(world, streams, oracle):
    """ops of lvl2_gate_batch and of ps_gate_batch_level"""
    K2 = world.need_ring(oracle)
    idx, K, _ = world.need_ps()
    st, = streams()
    api, r2, rp = world.api, world.ref("ring", 0), world.ref("ps", 0)
    count = 65
    ops2, opsp = pos.tile(r2["ops1"], count), pos.tile(rp["ops"], count)
    other2 = K2.gate_batch(sc.other_ops(r2["ops1"]), r2["a"], r2["b"])
    otherp = K.gate_batch(sc.other_ops(rp["ops"]), 0, rp["a"], rp["b"])
    L = Lane(world.eng, "lvl2_gate_batch and ps_gate_batch, ops overwritten", st)
    L.inp("a2", pos.tile(r2["a"], count))
    L.inp("b2", pos.tile(r2["b"], count))
    L.inp("ap", pos.tile(rp["a"], count))
    L.inp("bp", pos.tile(rp["b"], count))
    L.out("x2", r2["x1"], count)
    L.out("xp", rp["x1"], count)
    L.call("lvl2_gate_batch", lambda: api.lvl2_gate_batch(ops2, L.v("x2"), L.v("a2"), L.v("b2"), count=count, stream=st))
    L.call("ps_gate_batch", lambda: api.ps_gate_batch(idx, opsp, L.v("xp"), L.v("ap"), L.v("bp"), count=count, stream=st, level=0))
    overwritten_after_return(world, st, L, [ops2, opsp], [sc.other_ops(ops2), sc.other_ops(opsp)], [(r2["x1"], other2), (rp["x1"], otherp)])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. two and four streams with batch work in flight together
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [1, 2, 3], ids=["batch", "ll2", "ll"])
def test_two_gate_chains(world, streams, shape):
    """both lanes on one blind-rotation kernel; on the paired low-latency kernel (2) they share the device's fault word"""
    a, b = streams(2)
    with pos.options(world.api, dict(br_shape=shape)):
        run_lanes([gate_chain(world, a, 0, sc.SHORT_COUNTS), gate_chain(world, b, 1, sc.SHORT_COUNTS)])


@pytest.mark.parametrize("kernel", list(KS_KERNELS))
def test_two_keyswitch_chains(world, streams, kernel):
    a, b = streams(2)
    with pos.options(world.api, KS_KERNELS[kernel]):
        run_lanes([ks_chain(world, a, 0), ks_chain(world, b, 1)])


@pytest.mark.parametrize("cus", [0, 40], ids=["device", "cus40"])
def test_pack_beside_private_keyswitch(world, streams, cus):
    """one launch-shape rule, zero-then-add kernels on both sides; "cus_override" 40 cuts i into slices at these counts"""
    world.need_pks()
    a, b = streams(2)
    with pos.options(world.api, dict(cus_override=cus)):
        run_lanes([pack_chain(world, a, 0), pks_chain(world, b, 1)])


def test_lookup_beside_spread(world, streams):
    a, b = streams(2)
    run_lanes([lookup_chain(world, a, 0), spread_chain(world, b, 1)])


def test_two_trlwe_chains(world, streams):
    a, b = streams(2)
    run_lanes([trlwe_chain(world, a, 0, TRLWE_SHORT), trlwe_chain(world, b, 1, TRLWE_SHORT)])


@pytest.mark.parametrize("ks_mm", [1, 0], ids=["matrix-keyswitch", "rule-keyswitch"])
def test_two_linear_gate_chains_of_one_layer(world, streams, ks_mm):
    a, b = streams(2)
    with pos.options(world.api, dict(ks_mm_threshold=ks_mm)):
        run_lanes([linear_chain(world, a, 0), linear_chain(world, b, 1)])


def test_default_path_beside_the_ring(world, streams, oracle):
    world.need_ring(oracle)
    a, b = streams(2)
    run_lanes([gate_chain(world, a, 0, sc.SHORT_COUNTS), ring_chain(world, b, 1)])


def test_circuit_bootstraps_beside_the_extraction_chain(world, streams, oracle):
    """two lanes on the ring's kernels and on the private key switch at once"""
    world.need_ring_gate(oracle)
    world.need_pks()
    a, b = streams(2)
    run_lanes([cb_chain(world, a, 3), extract_chain(world, b, 0)])


def test_four_streams(world, streams):
    run_lanes([short_gate_chain(world, st, v, (1, 9, 65)) for v, st in enumerate(streams(4))])


def test_created_stream_beside_the_null_stream(world, streams):
    """created streams do not order against the null stream: neither lane waits for or disturbs the other"""
    a, = streams()
    run_lanes([gate_chain(world, a, 0, sc.SHORT_COUNTS), gate_chain(world, None, 1, sc.SHORT_COUNTS, label="null-stream gate chain")])


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. two issuing threads, a stream each
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_issuing_threads(world, streams):
    """each thread: its own stream and arena; eight times the short gate chain plus a rotation, a pack and a lookup, then its own
    stream's synchronise and every word.  ctypes releases the GIL around every library call."""
    sts = streams(2)
    lanes = []
    for v, st in enumerate(sts):
        L = short_gate_chain(world, st, v, (9, 65, 9), label="thread")
        api, r = world.api, world.ref("trlwe", v)
        c = 33
        e4 = pos.tile(r["e4"], c)
        m = np.arange(2 * c)
        dst, p = (m // 2).astype(np.int32), np.ascontiguousarray(r["pos6"][m % (2 * D)])
        L.inp("r3", pos.tile(r["r3"], c))
        L.inp("x5", pos.tile(r["x5"], 2 * c))
        L.inp("addr", pos.tile(r["addr"], c))
        L.inp("s7", pos.tile(r["s7"], c))
        L.out("r4", r["r4"], c)
        L.out("p6", r["p6"], c)
        L.out("o8", r["o8"], c)
        L.call("trlwe_rotate_batch", lambda L=L, st=st, e4=e4: api.trlwe_rotate_batch(L.v("r3"), e4, L.v("r4"), c, stream=st))
        L.call("pack_batch", lambda L=L, st=st, dst=dst, p=p: api.pack_batch(L.v("x5"), dst, p, L.v("p6"), 2 * c, c, stream=st))
        L.call("lut_lookup_batch", lambda L=L, st=st: api.lut_lookup_batch(L.v("addr"), L.v("s7"), L.v("o8"), c, c, nout=2, stream=st))
        lanes.append(L.build())
    results, go = [None, None], threading.Barrier(2)
    stop = threading.Event()

    def work(k):
        L, bad = lanes[k], []
        try:
            for rep in range(8):
                go.wait(timeout=60)
                if stop.is_set():
                    break
                if rep:
                    L.reset()
                for what, fn in L.calls:
                    if stop.is_set():           # the other thread met an error: nothing more is issued on the card
                        break
                    fn()
                if stop.is_set():
                    break
                rc = world.eng.lib.cufhe_amd_stream_synchronize(0, L.st)
                if rc != 0:
                    raise world.eng.CufheAmdError(f"cufhe_amd error {rc} from the stream's synchronise: {world.eng.lib.cufhe_amd_last_error().decode()}")
                bad += [f"repetition {rep}: {m}" for m in L.failures()]
            results[k] = bad
        except BaseException as e:          # noqa: B036 -- handed to the main thread, which decides
            stop.set()
            go.abort()
            results[k] = e
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join()
    finally:
        for L in lanes:
            L.close()
    for res in results:
        if isinstance(res, world.eng.CufheAmdError) and ("error -2" in str(res) or "synchronise" in str(res)):
            pytest.exit(f"two issuing threads: {res}", returncode=3)
        if isinstance(res, threading.BrokenBarrierError):
            continue
        if isinstance(res, BaseException):
            raise res
    bad = [m for res in results if isinstance(res, list) for m in res]
    assert not bad and all(isinstance(res, list) for res in results), "\n".join(bad) or repr(results)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. stream lifetime
# ---------------------------------------------------------------------------------------------------------------------------------
def test_destroy_without_a_synchronise_then_a_new_stream(world):
    """stream_destroy completes the stream's work: it returns 0 and every output is complete and right; a stream created afterwards
    (it may get the same handle) starts with no workspace and runs another chain"""
    api = world.api
    first = api.Stream(0)
    first.Create()
    handle = first.st().value
    L = gate_chain(world, first.st(), 0, sc.SHORT_COUNTS, label="destroyed without a synchronise").build()
    try:
        for i in range(len(L.calls)):
            L.issue(i)
        rc = world.eng.lib.cufhe_amd_stream_destroy(0, first.st())
        if rc != 0:
            pytest.exit(f"stream_destroy returned {rc}: {world.eng.lib.cufhe_amd_last_error().decode()}", returncode=3)
        bad = L.failures()
    finally:
        L.close()
    assert not bad, "\n".join(bad)
    second = api.Stream(0)
    second.Create()
    print(f"\n[stream contract] destroyed handle {handle:#x}, the next created stream has {second.st().value:#x}")
    try:
        with pos.options(api, dict(ks_mm_threshold=1)):
            run_lanes([linear_chain(world, second.st(), 1, label="on a stream created after the destroy")])
        run_lanes([trlwe_chain(world, second.st(), 1, TRLWE_SHORT, label="on a stream created after the destroy")])
    finally:
        second.Destroy()


LEAK_STREAMS, LEAK_SETS = 8, 1366        # 1366 sets * 3 rows * 1025 words * 4 bytes = 16.0 MiB of temporary per stream at level 1


def pooled_memory_round(world, din, dout):
    """eight live streams, linear_gate_batch with 16 MiB of temporary on each, all destroyed: the device's free memory afterwards"""
    api = world.api
    sts = []
    try:
        for _ in range(LEAK_STREAMS):
            s = api.Stream(0)
            s.Create()
            sts.append(s)
        for s in sts:
            device_call(world.eng, lambda s=s: api.linear_gate_batch(world.layer2, world.user1["op"], 1, dout, din, LEAK_SETS, stream=s.st()),
                        "linear_gate_batch with a large temporary")
    finally:
        for s in sts:
            s.Destroy()
    return api.device_mem_info()[0]


def test_stream_destroy_releases_the_linear_temporary(world, streams):
    """The temporary of linear_gate_batch is pooled per (device, stream).  stream_destroy releases it with the stream's workspace: after
    a round of eight streams with 16 MiB each the free memory is what it was before the round.  A library that kept the blocks until
    CleanUp would be 128 MiB short.  The bound is 1 MiB: on the MI355X two successive rounds of this build leave the same free memory to
    the byte (profiles/r29_stream_contract.md), and a kept block of any size a caller would notice shows.  A stream that stays alive
    runs the same call first, so that code objects and the pinned staging blocks exist before the first measurement."""
    api = world.api
    keep, = streams()
    din = api.DeviceBuffer(LEAK_SETS * 3 * W1).upload(rnd(9100, LEAK_SETS * 3 * W1))
    dout = api.DeviceBuffer(LEAK_SETS * 3 * W1)
    try:
        device_call(world.eng, lambda: api.linear_gate_batch(world.layer2, world.user1["op"], 1, dout, din, LEAK_SETS, stream=keep), "warm-up")
        synchronize(world.eng, keep, "warm-up")
        before = api.device_mem_info()[0]
        after1 = pooled_memory_round(world, din, dout)
        after2 = pooled_memory_round(world, din, dout)
    finally:
        din.free()
        dout.free()
    print(f"\n[stream contract] free memory before {before}, after one round {after1} ({before - after1:+d}), after two {after2} ({before - after2:+d})")
    block = LEAK_SETS * 3 * W1 * 4
    assert block >= 16 * sc.MIB - 65536
    assert before - after1 <= sc.MIB and before - after2 <= sc.MIB, \
        f"free memory fell by {before - after1} bytes over one round of {LEAK_STREAMS} destroyed streams and by {before - after2} over two: " \
        f"a pooled block of {block} bytes per stream was kept"
