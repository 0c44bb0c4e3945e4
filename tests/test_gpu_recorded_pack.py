"""GPU tests of the RECORDED pack (cufhe_amd_enqueue_pack / gPack / Pack).  Word parity is equality of every
word of every packed TRLWE with tests/pack_checker.py under a key of random words (parity needs no valid key), at the launch shapes
plan::plan_pack gives the node; one dependence level of five packs of mixed arity beside gates and a Spread is one zeroing launch and
one pack launch and writes nothing but its outputs; a dependent program without a fence against the in-order model
(tests/pack_program_model.py); the copying form; the RAM write of section 12 under a genuine key; the refusals.  The C++ mirror
tests/cpp/test_recorded_pack.cpp runs last."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import pack_checker as pk
import pack_program_model as pm
import packed_rom_checker as pr

pytestmark = pytest.mark.gpu

N, n = ol.N, ol.n
FILL = 0xA5A5A5A5
ARITIES = [1, 3, 4, 64, 65, 130]        # a single term, the three operands record_gate sees, one beyond, a full tile, one over, two tiles and a part
POSITIONS = (0, 1, 511, 1023)
SHAPES = (("pack_slices", 1), ("pack_slices", 40), ("pack_slices", -1), ("cus_override", 40))
POOL = 140                              # distinct input words of the parity tests: PackKS of each is computed once for the module
_loaded = [None]


def reinit(engine, keys):
    engine.CleanUp()                    # (releases the packing key and forgets lookup definitions)
    engine.SetGPUNum(1)
    engine.Initialize(keys.bk, keys.ksk)
    _loaded[0] = None


@pytest.fixture(scope="module", autouse=True)
def own_engine(engine, keys):
    """a freshly initialised engine for this file (no packing key yet: the first test needs that) and for the files that follow"""
    reinit(engine, keys)
    yield engine
    reinit(engine, keys)


def load_key(engine, name, key):
    if _loaded[0] != name:
        engine.api.pack_initialize(key)
        _loaded[0] = name


@pytest.fixture(scope="module")
def random_key_words():
    return np.random.default_rng(900).integers(0, 1 << 32, size=pk.KEY_WORDS, dtype=np.uint64).astype(np.uint32)


@pytest.fixture(scope="module")
def pool(random_key_words):
    """POOL lvl0 inputs with the edge words of the digit decomposition sown in, and the model that caches PackKS of each"""
    return pk.edge_inputs(np.random.default_rng(2700), POOL), pm.Model(random_key_words)


@pytest.fixture
def random_key(engine, random_key_words):
    load_key(engine, "random", random_key_words)
    return random_key_words


class Session:
    def __init__(self, eng, streams=1):
        self.eng, self.api = eng, eng.api
        self.st = []
        for _ in range(streams):
            s = self.api.Stream()
            s.Create()
            self.st.append(s)

    def ctxt(self, words=None, st=None, upload=True):
        c = self.api.Ctxt(0)
        c.tlwehost[:] = FILL if words is None else words
        if upload:
            self.api.CtxtCopyH2D(c, st or self.st[0])
        return c

    def trlwe(self, words=None, st=None):
        t = self.api.Trlwe()
        t.trlwehost[:] = FILL if words is None else words
        self.api.CtxtCopyH2D(t, st or self.st[0])
        return t

    def close(self):
        for s in self.st:
            s.Destroy()


def first_difference(got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return "%d words differ, first at %s" % (len(bad), int(bad[0]) if len(bad) else None)


def positions(rng, count):
    pos = np.array([POSITIONS[m % len(POSITIONS)] for m in range(count)], np.int32)
    pos[4::5] = rng.integers(0, N, size=len(pos[4::5]))
    return pos


def gates_recorded(api):
    return int(api.sched_stats().gates)


def test_refused_without_a_packing_key(own_engine, pool):
    """before cufhe_amd_pack_initialize on this (freshly initialised) device: -3, nothing recorded, the output untouched"""
    api, lib = own_engine.api, own_engine.lib
    assert _loaded[0] is None
    S = Session(own_engine)
    x = pool[0]
    ins = [S.ctxt(x[m]) for m in range(4)]
    out = S.trlwe()
    api.Synchronize()
    before = gates_recorded(api)
    arr = (ctypes.c_void_p * 4)(*[c._h for c in ins])
    p = np.zeros(4, np.int32)
    assert lib.cufhe_amd_enqueue_pack(0, S.st[0].st(), 0, out._h, 4, arr, p.ctypes.data) == -3
    assert b"cufhe_amd_pack_initialize" in lib.cufhe_amd_last_error()
    assert gates_recorded(api) == before
    api.CtxtCopyD2H(out, S.st[0])
    api.Synchronize()
    assert np.all(out.trlwehost == FILL)
    S.close()


@pytest.mark.parametrize("arity", ARITIES)
def test_one_pack_per_arity_at_every_shape(own_engine, random_key, pool, arity):
    """one recorded pack; the last term repeats the first term's handle and position (arity >= 2); "pack_slices" 1 and 40, the automatic
    rule and the rule at 40 CUs all give the checker's words, so the words are identical across shapes"""
    api = own_engine.api
    x, model = pool
    rng = np.random.default_rng(2800 + arity)
    idx = list(range(arity))
    pos = positions(rng, arity)
    if arity >= 2:
        idx[-1], pos[-1] = idx[0], pos[0]
    want = model.pack([x[i] for i in idx], pos)
    S = Session(own_engine)
    handles = {i: S.ctxt(x[i]) for i in sorted(set(idx))}
    out = S.trlwe()
    api.Synchronize()
    try:
        for key, value in SHAPES:
            api.set_option(key, value)
            out.trlwehost[:] = FILL
            api.CtxtCopyH2D(out, S.st[0])
            api.gPack(out, [handles[i] for i in idx], pos, S.st[0])
            api.CtxtCopyD2H(out, S.st[0])
            api.Synchronize()
            assert np.array_equal(out.trlwehost, want), f"{key} = {value}: " + first_difference(out.trlwehost, want)
            api.set_option(key, -1 if key == "pack_slices" else 0)
    finally:
        api.set_option("pack_slices", -1)
        api.set_option("cus_override", 0)
    for i, c in handles.items():          # the inputs are read, never written
        api.CtxtCopyD2H(c, S.st[0])
    api.Synchronize()
    assert all(np.array_equal(c.tlwehost, x[i]) for i, c in handles.items())
    S.close()


def pattern(words, tag):
    """guard words that depend on their position and on the guard (the idea of tests/footprint.py): a stray write of any constant, or of
    a neighbour's words, shows"""
    return ((np.arange(words, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(tag * 0x9E3779B1 + 0x5bd1e995)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def test_one_level_of_five_packs_is_two_launches(own_engine, keys, random_key_words, pool):
    """five packs of arities 1, 3, 64, 65, 7 in ONE dependence level (140 terms: the tiles of 64 straddle outputs; one input handle is
    shared by two packs) beside 8 NAND gates and a recorded Spread: every word equals its checker; the level is one launch sequence of
    the gates plus one pack lowering (one zeroing launch and one kernel launch, a single profiled launcher call); the guard TRLWEs
    that lie between the outputs in device memory, the guard ciphertexts between the inputs and the inputs keep their words"""
    import lut_checker as lc
    load_key(own_engine, "random", random_key_words)
    api, lib = own_engine.api, own_engine.lib
    x, model = pool
    S = Session(own_engine, streams=4)
    arities = [1, 3, 64, 65, 7]
    rng = np.random.default_rng(2900)
    # TRLWE slots are 8 KiB with nothing between them: of 24 handles sorted by device address, an output is one whose two neighbours in
    # memory are handles too, and those neighbours are its guards
    ptr = lambda c: lib.cufhe_amd_ctxt_device_ptr(c._h, 0)
    ts = sorted((api.Trlwe() for _ in range(24)), key=ptr)
    out_at = []
    for i in range(1, len(ts) - 1):
        if len(out_at) < 5 and (not out_at or i >= out_at[-1] + 2) and ptr(ts[i]) - ptr(ts[i - 1]) == 8 * N and ptr(ts[i + 1]) - ptr(ts[i]) == 8 * N:
            out_at.append(i)
    assert len(out_at) == 5, "no five TRLWE slots with handles on both sides"
    outs = [ts[i] for i in out_at]
    guard_tag = {i: i for i in range(len(ts)) if i not in out_at}
    for i, t in enumerate(ts):
        t.trlwehost[:] = FILL if i in out_at else pattern(2 * N, guard_tag[i])
        api.CtxtCopyH2D(t, S.st[0])
    guards_t = [ts[i] for i in guard_tag]
    # lvl0 inputs with a guard ciphertext after every eighth
    handles, guards_c = [], []
    for i in range(POOL):
        handles.append(S.ctxt(x[i], S.st[i % 4]))
        if i % 8 == 7:
            guards_c.append(S.ctxt(pattern(n + 1, 100 + i)))
    spread_in, spread_out = S.trlwe(pattern(2 * N, 50)), S.trlwe()
    bits = rng.integers(0, 2, size=(2, 8)).astype(np.uint8)
    ea, eb = keys.encrypt(bits[0], 0, seed=2901), keys.encrypt(bits[1], 0, seed=2902)
    ga, gb, go = [S.ctxt(ea[g]) for g in range(8)], [S.ctxt(eb[g]) for g in range(8)], [S.ctxt() for _ in range(8)]
    api.Synchronize()
    terms, first = [], 0
    for k, a in enumerate(arities):
        idx = list(range(first, first + a))
        first += a - 1                          # the last handle of a pack is the first of the next: shared by two packs
        pos = positions(rng, a)
        if a >= 2:
            pos[1] = pos[0]                     # two terms at one position
        terms.append((idx, pos))
    assert first + 1 <= POOL and sum(arities) == 140
    api.sched_stats(reset=True)
    api.profile_enable(True)
    try:
        api.profile_get(reset=True)
        for k, (idx, pos) in enumerate(terms):      # interleaved with the gates, on several streams
            api.gPack(outs[k], [handles[i] for i in idx], pos, S.st[k % 4])
            api.gNand(go[k], ga[k], gb[k], S.st[(k + 1) % 4])
        api.gSpread(spread_out, spread_in, 2, 128, S.st[0])
        for g in range(5, 8):
            api.gNand(go[g], ga[g], gb[g], S.st[g % 4])
        for c in outs + guards_t + [spread_out] + go + guards_c + handles:
            api.CtxtCopyD2H(c, S.st[0])
        api.Synchronize()
        stats = api.sched_stats()
        prof = api.profile_get(reset=True)
    finally:
        api.profile_enable(False)
    for k, (idx, pos) in enumerate(terms):
        want = model.pack([x[i] for i in idx], pos)
        assert np.array_equal(outs[k].trlwehost, want), (k, first_difference(outs[k].trlwehost, want))
    assert np.array_equal(np.stack([c.tlwehost for c in go]), keys.gate_batch(api.NAND, 0, ea, eb))
    assert np.array_equal(spread_out.trlwehost, lc.spread(pattern(2 * N, 50), 2, 128))
    assert stats.gates == 5 + 8 + 1 and stats.levels == 1, (stats.gates, stats.levels)
    # what was really launched (the library's profiling events, one pair per launcher call): the gates' rotation and key switch, and ONE
    # pack lowering over all 140 terms
    assert prof.blind_rotate_launches == 1 and prof.blind_rotations == 8, (prof.blind_rotate_launches, prof.blind_rotations)
    assert prof.keyswitch_launches == 2 and prof.keyswitches == 8 + 140, (prof.keyswitch_launches, prof.keyswitches)
    for i in guard_tag:
        assert np.array_equal(ts[i].trlwehost, pattern(2 * N, i)), ("TRLWE guard", i, first_difference(ts[i].trlwehost, pattern(2 * N, i)))
    for j, g in enumerate(guards_c):
        assert np.array_equal(g.tlwehost, pattern(n + 1, 100 + 8 * j + 7)), ("lvl0 guard", j)
    assert all(np.array_equal(handles[i].tlwehost, x[i]) for i in range(POOL))
    S.close()


_dependent = {}


@pytest.mark.parametrize("rename", [0, 1])
def test_dependent_program_without_a_fence(own_engine, keys, random_key, pool, rename):
    """gates -> gPack -> gSpread -> gLookup -> D2H with nothing but the final Synchronize: the pack waits for the gates that make its
    inputs, the Spread and a lookup read the packed TRLWE, a SECOND pack goes into the same TRLWE after they are recorded (write after
    read on a table), and a gate overwrites input 5 of the first pack after it is recorded.  Every value equals the in-order model."""
    api = own_engine.api
    x, _ = pool
    model = pm.Model(random_key, keys)
    c0 = [x[i] for i in range(24)]                       # slots 0 .. 15 operands, 16 .. 23 the gate results, slot 15 also the lookup address
    prog = [{"kind": "nand", "out": 16 + k, "a": 2 * k, "b": 2 * k + 1} for k in range(8)]
    prog.append({"kind": "pack", "tout": 0, "ins": [16, 17, 18, 19, 20, 21, 22, 23, 16], "pos": [0, 128, 256, 384, 512, 640, 768, 896, 0]})
    prog.append({"kind": "spread", "tout": 1, "tin": 0, "stride": 1, "reps": 128})
    prog.append({"kind": "lookup", "out": 0, "table": 1, "a": 15})
    prog.append({"kind": "lookup", "out": 1, "table": 0, "a": 15})
    prog.append({"kind": "pack", "tout": 0, "ins": [2, 3, 4, 5, 6], "pos": [1, 1, 2, 3, 1023]})
    prog.append({"kind": "nand", "out": 21, "a": 8, "b": 9})       # input 5 of the first pack
    if "want" not in _dependent:             # the model's two lookups are CPU blind rotations: once for both cases
        _dependent["want"] = model.run(c0, [np.full(2 * N, FILL, np.uint32)] * 2, prog)
    want_c, want_t = _dependent["want"]
    api.set_option("sched_rename", rename)
    try:
        S = Session(own_engine, streams=2)
        c = [S.ctxt(w, S.st[i % 2]) for i, w in enumerate(c0)]
        t = [S.trlwe(), S.trlwe()]
        op = api.DefineLookup((1, 0), 0, 1)
        for j, o in enumerate(prog):
            st = S.st[j % 2]
            if o["kind"] == "nand":
                api.gNand(c[o["out"]], c[o["a"]], c[o["b"]], st)
            elif o["kind"] == "pack":
                api.gPack(t[o["tout"]], [c[i] for i in o["ins"]], o["pos"], st)
            elif o["kind"] == "spread":
                api.gSpread(t[o["tout"]], t[o["tin"]], o["stride"], o["reps"], st)
            else:
                api.gLookup([c[o["out"]]], t[o["table"]], c[o["a"]], None, op, st)
        for h in c + t:
            api.CtxtCopyD2H(h, S.st[0])
        api.Synchronize()
    finally:
        api.set_option("sched_rename", 1)
    for i in range(2):
        assert np.array_equal(t[i].trlwehost, want_t[i]), ("TRLWE", i, first_difference(t[i].trlwehost, want_t[i]))
    for i in range(24):
        assert np.array_equal(c[i].tlwehost, want_c[i]), ("ciphertext", i, first_difference(c[i].tlwehost, want_c[i]))
    S.close()


def test_copying_form(own_engine, random_key, pool):
    """Pack: the inputs come from their host words (never uploaded by the test), the result is in out's host words once StreamQuery
    says so"""
    api = own_engine.api
    x, model = pool
    S = Session(own_engine)
    idx, pos = [7, 8, 9, 10, 11, 7], [5, 6, 7, 8, 9, 5]
    handles = {i: S.ctxt(x[i], upload=False) for i in set(idx)}
    out = api.Trlwe()
    out.trlwehost[:] = FILL
    api.Pack(out, [handles[i] for i in idx], pos, S.st[0])
    while not api.StreamQuery(S.st[0]):
        pass
    want = model.pack([x[i] for i in idx], pos)
    assert np.array_equal(out.trlwehost, want), first_difference(out.trlwehost, want)
    S.close()


def test_refused_with_a_parameter_set_active(own_engine, keys, random_key, pool):
    api, lib = own_engine.api, own_engine.lib
    S = Session(own_engine)
    ins = [S.ctxt(pool[0][m]) for m in range(4)]
    out = S.trlwe()
    api.Synchronize()
    arr = (ctypes.c_void_p * 4)(*[c._h for c in ins])
    p = np.zeros(4, np.int32)
    ps = api.ps_index("default")
    api.ps_initialize(ps, keys.bk, keys.ksk)
    before = gates_recorded(api)
    api.set_option("param_set", ps)
    try:
        assert lib.cufhe_amd_enqueue_pack(0, S.st[0].st(), 0, out._h, 4, arr, p.ctypes.data) == -1
        assert b"param_set" in lib.cufhe_amd_last_error()
    finally:
        api.set_option("param_set", -1)
    assert gates_recorded(api) == before
    api.CtxtCopyD2H(out, S.st[0])
    api.Synchronize()
    assert np.all(out.trlwehost == FILL)
    S.close()


def word_trlwe(keys, word, seed):
    """a host-encrypted TRLWE with bit b of `word` at coefficient b, messages +-mu"""
    msgs = np.zeros(N, np.uint32)
    for b in range(8):
        msgs[b] = ol.MU if (word >> b) & 1 else (1 << 32) - ol.MU
    return pr.encrypt_trlwe(keys, msgs, 64.0, seed)


def test_ram_write_end_to_end(own_engine, keys):
    """the RAM write of INTEGRATION.md section 12 written with gPack under a genuine key: eight recorded Xor gates, the recorded pack of
    their results at coefficients 0 .. 7, gCMUXNTT against the stored word under a write-enable selector, indexed extraction -- no fence
    and no wait before the final Synchronize.  The packed words equal the checker's, the decrypted word is the new one for write-enable
    1 and the old one for 0 (the noise claim of section 12 stands: the words are the batch call's)."""
    api = own_engine.api
    key = pk.genuine_key(keys, seed=901)
    load_key(own_engine, "genuine", key)
    rng = np.random.default_rng(3000)
    a, b = rng.integers(0, 2, size=(2, 8)).astype(np.uint8)
    old = int(rng.integers(0, 256))
    ea, eb = keys.encrypt(a, 0, seed=3001), keys.encrypt(b, 0, seed=3002)
    S = Session(own_engine)
    st = S.st[0]
    for we in (1, 0):
        ca, cb, cx = [S.ctxt(ea[k]) for k in range(8)], [S.ctxt(eb[k]) for k in range(8)], [S.ctxt() for _ in range(8)]
        new, cell = S.trlwe(), S.trlwe()
        cell_old = S.trlwe(word_trlwe(keys, old, seed=3003))
        sel = api.TrgswNtt()
        api.TRGSW2NTT(sel, pr.selector(keys, we), st)
        for k in range(8):
            api.gXor(cx[k], ca[k], cb[k], st)
        api.gPack(new, cx, list(range(8)), st)
        api.gCMUXNTT(cell, sel, new, cell_old, st)
        outs = [S.ctxt(upload=False) for _ in range(8)]
        for k in range(8):
            api.gSampleExtractAndKeySwitch(outs[k], cell, st, index=k)
            api.CtxtCopyD2H(outs[k], st)
        for h in cx + [new]:
            api.CtxtCopyD2H(h, st)
        api.Synchronize()
        gates = np.stack([c.tlwehost for c in cx])
        assert list(keys.decrypt(gates, 0)) == list(a ^ b)
        assert np.array_equal(new.trlwehost, pk.pack_batch(key, gates, np.zeros(8, np.int32), np.arange(8), 1)[0])
        got = keys.decrypt(np.stack([o.tlwehost for o in outs]), 0)
        want = (a ^ b) if we else np.array([(old >> k) & 1 for k in range(8)], np.uint8)
        assert list(got) == list(want), f"write-enable {we}"
    S.close()


def build_cpp_program():
    """tests/cpp/test_recorded_pack.cpp -> tests/cpp/test_recorded_pack, with the flags tests/cpp_build.py gives the other C++ programs"""
    import cpp_build
    cdefs, libs = cpp_build.hip_flags()
    root = ol.ROOT
    exe = os.path.join(root, "tests", "cpp", "test_recorded_pack")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + cdefs +
                          ["-o", exe, os.path.join(root, "tests", "cpp", "test_recorded_pack.cpp"),
                           "-L" + os.path.join(root, "cufhe_amd"), "-lcufhe_amd", "-L" + os.path.join(root, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(root, "cufhe_amd"), "-Wl,-rpath," + os.path.join(root, "oracle")] + libs)
    return exe


def test_cpp_recorded_pack(own_engine, keys):
    """tests/cpp/test_recorded_pack.cpp: the RAM write through gPack / Pack of include/cufhe_amd.hpp"""
    exe = build_cpp_program()
    own_engine.CleanUp()                  # the C++ program owns the device state while it runs
    _loaded[0] = None
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        own_engine.SetGPUNum(1)
        own_engine.Initialize(keys.bk, keys.ksk)
