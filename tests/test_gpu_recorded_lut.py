"""GPU tests of the RECORDED lookups, Spreads and table rotations (cufhe_amd_enqueue_lookup / _enqueue_spread / _enqueue_lut_rotate,
INTEGRATION.md section 13): every word equals tests/lookup_program_model.py on random words (parity needs no valid ciphertext) on
every blind-rotate kernel and across the segments of one launch; all recorded lookups of a dependence level are ONE launch sequence;
sibling groups cost one rotation; Spread descriptors carry their own (stride, reps); random dependent programs; the worked example
under genuine keys; the refusals.  The sizes are those of tests/test_gpu_lut.py."""
import os
import subprocess

import numpy as np
import pytest

import lookup_program_model as lm
import lut_checker as lc
import oracle_lib as ol
import packed_rom_checker as pr
import user_gate_checker as uc
from test_gpu_user_gates import set_shape, up

pytestmark = pytest.mark.gpu

N, n = ol.N, ol.n
MU = ol.MU
FILL = 0xA5A5A5A5
SHAPES = ["batch", "half", "ll", "ll2"]
TABLES, PAIRS, ROTATIONS = 5, 7, 19
DEF_A = (1, 0, 0)                       # the address is in0: cufhe_amd_lut_lookup_batch's words
DEF_B = (1, 1, 0x2468ACE1)              # two operands and an offset
PAIR_NOUT = (1, 2, 8, 1, 2, 8, 1)       # the 7 pairs mix nout 1, 2, 8 ...
PAIR_DEF = ("A", "B", "A", "B", "A", "B", "A")      # ... and the two definitions


def reinit(engine, keys):
    engine.CleanUp()
    engine.SetGPUNum(1)
    engine.Initialize(keys.bk, keys.ksk)


@pytest.fixture
def fresh(engine, keys):
    """a freshly initialised engine before and after: no definitions left behind for the files that follow"""
    reinit(engine, keys)
    yield engine
    reinit(engine, keys)


class Data:
    """test_gpu_lut.py's 5 tables and 7 address ciphertexts in 7 distinct pairs; pair q under definition B adds ciphertext q + 1.  The
    model's outputs are computed once per (pair, table, definition, nout), on threads, and shared by the tests."""

    def __init__(self, keys):
        rng = np.random.default_rng(1600)
        self.keys = keys
        self.tables = rng.integers(0, 1 << 32, size=(TABLES, 2 * N), dtype=np.uint64).astype(np.uint32)
        self.x = rng.integers(0, 1 << 32, size=(PAIRS, n + 1), dtype=np.uint64).astype(np.uint32)
        self.x[0, n] = 0
        self.x[1, n] = 0xFFFFFFFF
        self.pair_table = np.array([g % TABLES for g in range(PAIRS)], np.int32)
        self._ref = {}

    def second(self, q):
        return (q + 1) % PAIRS

    def refs(self, wanted):
        """{(q, table, def, nout): [nout][n + 1]} for every key in `wanted`"""
        todo = [k for k in dict.fromkeys(wanted) if k not in self._ref]

        def one(i):
            q, t, d, nout = todo[i]
            c = DEF_A if d == "A" else DEF_B
            return lm.lookup(self.keys, c + (nout,), self.tables[t], self.x[q], self.x[self.second(q)])
        for k, r in zip(todo, lc.on_threads(one, len(todo))):
            self._ref[k] = r
        return {k: self._ref[k] for k in wanted}


@pytest.fixture(scope="module")
def data(keys):
    return Data(keys)


class Session:
    """definitions and streams of one test, on a freshly initialised engine"""

    def __init__(self, eng, streams=1):
        self.eng, self.api = eng, eng.api
        self.ops = {}
        self.st = []
        for _ in range(streams):
            s = self.api.Stream()
            s.Create()
            self.st.append(s)

    def op(self, d, nout):
        if (d, nout) not in self.ops:
            c = DEF_A if d == "A" else DEF_B
            self.ops[(d, nout)] = self.api.DefineLookup(c[:2], c[2], nout)
        return self.ops[(d, nout)]

    def ctxt(self, words, st=None):
        c = self.api.Ctxt(0)
        if words is None:
            c.tlwehost[:] = FILL
        else:
            c.tlwehost[:] = words
        self.api.CtxtCopyH2D(c, st or self.st[0])
        return c

    def trlwe(self, words, st=None):
        t = self.api.Trlwe()
        t.trlwehost[:] = FILL if words is None else words
        self.api.CtxtCopyH2D(t, st or self.st[0])
        return t

    def close(self):
        for s in self.st:
            s.Destroy()


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "%d words differ, first at (row, word) %s" % (len(bad), tuple(bad[0]) if len(bad) else None)


def record_items(S, data, items, tabs, streams=None):
    """items: (pair, table, def, nout) each with address handles of its OWN (equal words in different buffers are different
    evaluations).  Returns the output handles per item."""
    api = S.api
    outs = []
    for i, (q, t, d, nout) in enumerate(items):
        st = S.st[i % len(S.st)] if streams is None else streams[i]
        a = S.ctxt(data.x[q], st)
        b = S.ctxt(data.x[data.second(q)], st) if d == "B" else None
        o = [S.ctxt(None, st) for _ in range(nout)]
        outs.append((st, a, b, o))
    api.Synchronize()              # operands are on the device: what follows is the lookups alone
    return outs


def issue(S, items, tabs, handles, copy_back=True):
    api = S.api
    for (q, t, d, nout), (st, a, b, o) in zip(items, handles):
        api.gLookup(o, tabs[t], a, b, S.op(d, nout), st)
    if copy_back:
        for st, a, b, o in handles:
            for c in o:
                api.CtxtCopyD2H(c, st)


def check_items(data, items, handles):
    want = data.refs(items)
    for i, (key, (st, a, b, o)) in enumerate(zip(items, handles)):
        got = np.stack([c.tlwehost for c in o])
        assert np.array_equal(got, want[key]), (i, key, first_difference(got, want[key]))


def pair_item(data, q):
    return (q, int(data.pair_table[q]), PAIR_DEF[q], PAIR_NOUT[q])


@pytest.mark.parametrize("shape", SHAPES)
def test_lookup_words_on_every_kernel(fresh, data, shape):
    """19 recorded lookups tiled from the 7 pairs in ONE dependence level -- three workgroups of 8 with idle waves in the last, five
    of 4, an odd count for the paired kernel -- mixing nout 1, 2, 8 and the definitions (1, 0) offset 0 and (1, 1) with an offset:
    every output word equals the model's"""
    S = Session(fresh)
    items = [pair_item(data, g % PAIRS) for g in range(ROTATIONS)]
    assert {i[3] for i in items} == {1, 2, 8} and {i[2] for i in items} == {"A", "B"}
    tabs = [S.trlwe(data.tables[t]) for t in range(TABLES)]
    handles = record_items(S, data, items, tabs)
    set_shape(S.api, shape)
    try:
        S.api.sched_stats(reset=True)
        issue(S, items, tabs, handles)
        S.api.Synchronize()
        stats = S.api.sched_stats()
    finally:
        set_shape(S.api, None)
    check_items(data, items, handles)
    assert stats.levels == 1 and stats.launch_sequences == 1, (stats.levels, stats.launch_sequences)
    for t in range(TABLES):       # the tables are read, never written
        S.api.CtxtCopyD2H(tabs[t], S.st[0])
    S.api.Synchronize()
    assert all(np.array_equal(tabs[t].trlwehost, data.tables[t]) for t in range(TABLES))
    S.close()


def test_one_launch_sequence_per_level(fresh, keys, data):
    """64 recorded single-output lookups issued on 8 streams are ONE dependence level and ONE launch sequence; with 64 NANDs beside
    them, one level and two sequences (the gates' and the lookups').  The words are the model's in both runs."""
    S = Session(fresh, streams=8)
    api = S.api
    singles = [q for q in range(PAIRS) if PAIR_NOUT[q] == 1]
    items = [pair_item(data, singles[g % len(singles)]) for g in range(64)]
    tabs = [S.trlwe(data.tables[t]) for t in range(TABLES)]
    handles = record_items(S, data, items, tabs)
    bits = np.random.default_rng(2100).integers(0, 2, size=(2, 64)).astype(np.uint8)
    ea, eb = keys.encrypt(bits[0], 0, seed=2101), keys.encrypt(bits[1], 0, seed=2102)
    ga, gb, go = [S.ctxt(ea[g], S.st[g % 8]) for g in range(64)], [S.ctxt(eb[g], S.st[g % 8]) for g in range(64)], [S.ctxt(None) for _ in range(64)]
    api.Synchronize()
    for with_gates, sequences in ((False, 1), (True, 2)):
        for st, a, b, o in handles:
            o[0].tlwehost[:] = FILL
        api.sched_stats(reset=True)
        api.profile_enable(True)
        api.profile_get(reset=True)
        for g in range(64):      # interleaved, the way a netlist issues them
            (q, t, d, nout), (st, a, b, o) = items[g], handles[g]
            api.gLookup(o, tabs[t], a, b, S.op(d, nout), st)
            if with_gates:
                api.gNand(go[g], ga[g], gb[g], S.st[g % 8])
        for st, a, b, o in handles:
            api.CtxtCopyD2H(o[0], st)
        if with_gates:
            for g in range(64):
                api.CtxtCopyD2H(go[g], S.st[g % 8])
        api.Synchronize()
        stats = api.sched_stats()
        prof = api.profile_get(reset=True)
        api.profile_enable(False)
        assert stats.levels == 1 and stats.launch_sequences == sequences, (with_gates, stats.levels, stats.launch_sequences)
        # and what was really launched (the library's profiling events, one pair per launcher call): one rotation launch and one
        # key-switch launch per sequence
        assert (prof.blind_rotate_launches, prof.keyswitch_launches) == (sequences, sequences), (prof.blind_rotate_launches, prof.keyswitch_launches)
        assert (prof.blind_rotations, prof.keyswitches) == (64 * sequences, 64 * sequences)
        check_items(data, items, handles)
        if with_gates:
            assert np.array_equal(np.stack([c.tlwehost for c in go]), keys.gate_batch(api.NAND, 0, ea, eb))
    S.close()


def test_every_segment_reads_its_own_tables(fresh, data):
    """8 cus + 5 recorded lookups under the default rules, test_gpu_lut.py's pairing: one full round of the batch kernel and a tail
    segment on another kernel.  Every row equals the model's: the table-pointer array across plan segments, through the recorded path"""
    S = Session(fresh, streams=4)
    count = 8 * S.api.device_cus() + 5
    pair = (np.arange(count) * 3 + 1) % PAIRS
    assert not np.array_equal(pair[:5], pair[-5:])
    items = [(int(q), int(data.pair_table[q]), "A", 1) for q in pair]
    tabs = [S.trlwe(data.tables[t]) for t in range(TABLES)]
    handles = record_items(S, data, items, tabs)
    # an idle device is handed a level as soon as it holds one grid round: keep the level together, so that ONE launch spans the segments
    S.api.set_option("sched_idle_gates", count + 1)
    try:
        S.api.sched_stats(reset=True)
        issue(S, items, tabs, handles)
        S.api.Synchronize()
        stats = S.api.sched_stats()
    finally:
        S.api.set_option("sched_idle_gates", -1)
    check_items(data, items, handles)
    assert stats.levels == 1 and stats.launch_sequences == 1 and stats.max_level_gates == count, (stats.levels, stats.launch_sequences)
    S.close()


def rotations_of(api, fn):
    """blind rotations and key switches launched while fn() runs and completes"""
    api.profile_enable(True)
    try:
        api.profile_get(reset=True)
        fn()
        api.Synchronize()
        p = api.profile_get(reset=True)
    finally:
        api.profile_enable(False)
    return int(p.blind_rotations), int(p.keyswitches)


def test_sibling_groups_cost_one_rotation(fresh, data):
    """a full nout = 8 group: one rotation, eight key switches; the same evaluation recorded twice in one level (16 outputs): still one
    rotation; a group requested as outputs {5, 0, 3} only: one rotation, three key switches; two groups of one definition on different
    tables in one level: two rotations.  Every word equals the model's."""
    S = Session(fresh)
    api = S.api
    tabs = [S.trlwe(data.tables[t]) for t in range(TABLES)]
    op = S.op("A", 8)
    a = S.ctxt(data.x[2])
    o1, o2, o3 = ([S.ctxt(None) for _ in range(8)] for _ in range(3))
    api.Synchronize()
    want = data.refs([(2, 2, "A", 8), (2, 3, "A", 8)])

    def copy_back(*groups):
        for g in groups:
            for c in g:
                api.CtxtCopyD2H(c, S.st[0])

    assert rotations_of(api, lambda: (api.gLookup(o1, tabs[2], a, None, op, S.st[0]), copy_back(o1))) == (1, 8)
    assert np.array_equal(np.stack([c.tlwehost for c in o1]), want[(2, 2, "A", 8)])
    # the same evaluation twice, the second time into other handles: fused by (definition, in0, in1, table)
    assert rotations_of(api, lambda: (api.gLookup(o1, tabs[2], a, None, op, S.st[0]), api.gLookup(o2, tabs[2], a, None, op, S.st[0]),
                                      copy_back(o1, o2))) == (1, 16)
    assert np.array_equal(np.stack([c.tlwehost for c in o2]), want[(2, 2, "A", 8)])
    # a group requested as outputs {5, 0, 3} only, in that order: output 5 by one call, outputs 0 and 3 by the next (None: not requested).
    # The level's list names the siblings 5, 0, 3; they are fused whatever their order: one rotation, three key switches
    p5, p0, p3 = (S.ctxt(None) for _ in range(3))
    api.Synchronize()
    only5 = [None] * 5 + [p5] + [None] * 2
    only03 = [p0, None, None, p3] + [None] * 4
    api.sched_stats(reset=True)
    assert rotations_of(api, lambda: (api.gLookup(only5, tabs[2], a, None, op, S.st[0]), api.gLookup(only03, tabs[2], a, None, op, S.st[0]),
                                      copy_back([p5, p0, p3]))) == (1, 3)
    assert api.sched_stats().levels == 1 and api.sched_stats().gates == 3
    for c, j in ((p5, 5), (p0, 0), (p3, 3)):
        assert np.array_equal(c.tlwehost, want[(2, 2, "A", 8)][j]), j
    # and in one call
    for c in (p5, p0, p3):
        c.tlwehost[:] = FILL
    assert rotations_of(api, lambda: (api.gLookup([p0, None, None, p3, None, p5, None, None], tabs[2], a, None, op, S.st[0]),
                                      copy_back([p5, p0, p3]))) == (1, 3)
    for c, j in ((p5, 5), (p0, 0), (p3, 3)):
        assert np.array_equal(c.tlwehost, want[(2, 2, "A", 8)][j]), j
    # one definition, one address, two tables: two evaluations in one level
    api.sched_stats(reset=True)
    assert rotations_of(api, lambda: (api.gLookup(o1, tabs[2], a, None, op, S.st[0]), api.gLookup(o3, tabs[3], a, None, op, S.st[0]),
                                      copy_back(o1, o3))) == (2, 16)
    assert api.sched_stats().levels == 1
    assert np.array_equal(np.stack([c.tlwehost for c in o1]), want[(2, 2, "A", 8)])
    assert np.array_equal(np.stack([c.tlwehost for c in o3]), want[(2, 3, "A", 8)])
    S.close()


SPREAD_SHAPES = [(1, 256), (2, 128), (8, 16), (1, 1), (1024, 1), (1, 1024)]
_spread_ref = {}


def spread_reference():
    """5 random TRLWEs and the checker's Spread of each under each of the six shapes, once"""
    if not _spread_ref:
        c = np.random.default_rng(1800).integers(0, 1 << 32, size=(5, 2 * N), dtype=np.uint64).astype(np.uint32)
        _spread_ref["in"] = c
        for sh in SPREAD_SHAPES:
            _spread_ref[sh] = np.stack([lc.spread(c[g], *sh) for g in range(5)])
    return _spread_ref


@pytest.mark.parametrize("count", [1, 5, 65])
def test_spread_descriptors(fresh, count):
    """recorded Spreads in ONE level, a DIFFERENT (stride, reps) per item: the checker's words, and cufhe_amd_trlwe_spread_batch's on
    the same inputs item by item.  65 TRLWEs are 33 workgroups, the last with two idle waves."""
    S = Session(fresh)
    api = S.api
    ref = spread_reference()
    ins = [S.trlwe(ref["in"][g]) for g in range(5)]
    outs = [S.trlwe(None) for _ in range(count)]
    api.Synchronize()
    shapes = [SPREAD_SHAPES[(g + 2 * (g // 5)) % len(SPREAD_SHAPES)] for g in range(count)]
    if count > 1:
        assert len(set(shapes)) == min(count, len(SPREAD_SHAPES))
    api.sched_stats(reset=True)
    for g in range(count):
        api.gSpread(outs[g], ins[g % 5], shapes[g][0], shapes[g][1], S.st[0])
        api.CtxtCopyD2H(outs[g], S.st[0])
    api.Synchronize()
    stats = api.sched_stats()
    assert stats.levels == 1 and stats.launch_sequences == 1, (stats.levels, stats.launch_sequences)
    dout = up(fresh, np.full(2 * N, FILL, np.uint32))
    for g in range(count):
        want = ref[shapes[g]][g % 5]
        assert np.array_equal(outs[g].trlwehost, want), (g, shapes[g], first_difference(outs[g].trlwehost[None], want[None]))
    for sh in set(shapes):        # the batch call on the same inputs, item by item
        for g in range(5):
            api.trlwe_spread_batch(up(fresh, ref["in"][g]), dout, 1, sh[0], sh[1])
            fresh.Synchronize()
            assert np.array_equal(dout.download(), ref[sh][g]), (sh, g)
    S.close()


def test_recorded_table_rotation(fresh, data):
    """LUT_ROTATE beside lookups in one level: the accumulator after all n steps, extracted by a recorded SampleExtractAndKeySwitch, is
    the lookup's output 0 -- the model's words -- and the accumulator is the checker's"""
    S = Session(fresh)
    api = S.api
    tabs = [S.trlwe(data.tables[t]) for t in range(TABLES)]
    accs = [S.trlwe(None) for _ in range(3)]
    addrs = [S.ctxt(data.x[q]) for q in (0, 3, 6)]
    outs = [S.ctxt(None) for _ in range(3)]
    look = [S.ctxt(None) for _ in range(3)]
    api.Synchronize()
    op = S.op("A", 1)
    for i, q in enumerate((0, 3, 6)):
        t = tabs[int(data.pair_table[q])]
        api.gLutRotate(accs[i], t, addrs[i], S.st[0])
        api.gLookup([look[i]], t, addrs[i], None, op, S.st[0])
        api.gSampleExtractAndKeySwitch(outs[i], accs[i], S.st[0], index=0)
        for c in (accs[i], outs[i], look[i]):
            api.CtxtCopyD2H(c, S.st[0])
    api.Synchronize()
    want = data.refs([(q, int(data.pair_table[q]), "A", 1) for q in (0, 3, 6)])
    for i, q in enumerate((0, 3, 6)):
        w = want[(q, int(data.pair_table[q]), "A", 1)][0]
        assert np.array_equal(look[i].tlwehost, w) and np.array_equal(outs[i].tlwehost, w), (q,)
    assert np.array_equal(accs[0].trlwehost, lm.lut_rotate(data.keys, data.tables[int(data.pair_table[0])], data.x[0]))
    S.close()


def test_copying_form(fresh, data):
    """Lookup (copying): the address operands AND the table come from their host members, the results land in the outputs' host members
    after Synchronize() -- no CtxtCopyH2D / D2H by the caller.  One- and two-operand definitions, nout 1 and 2."""
    S = Session(fresh)
    api = S.api
    st = S.st[0]
    for q in (0, 1):
        key = pair_item(data, q)
        _, t, d, nout = key
        table, a, b = api.Trlwe(), api.Ctxt(0), api.Ctxt(0)
        table.trlwehost[:] = data.tables[t]
        a.tlwehost[:] = data.x[q]
        b.tlwehost[:] = data.x[data.second(q)]
        outs = [api.Ctxt(0) for _ in range(nout)]
        api.Lookup(outs, table, a, b if d == "B" else None, S.op(d, nout), st)
        api.Synchronize()
        want = data.refs([key])[key]
        got = np.stack([c.tlwehost for c in outs])
        assert np.array_equal(got, want), (key, first_difference(got, want))
    S.close()


# ---- random dependent programs ----
PROGRAMS, PROGRAM_OPS = 20, 40
_program_ref = {}


def program_references(keys):
    """the 20 programs and the model's final values, computed once (programs on threads) and shared by the four configurations"""
    if not _program_ref:
        progs = [lm.generate(2400 + i, PROGRAM_OPS) for i in range(PROGRAMS)]
        finals = lc.on_threads(lambda i: lm.evaluate(keys, *progs[i]), PROGRAMS)
        _program_ref["progs"], _program_ref["finals"] = progs, finals
    return _program_ref["progs"], _program_ref["finals"]


def run_program(S, lookups, user_op, init_c, init_t, prog):
    """issue a program through the per-gate API on device buffers, on two streams in turn; returns the final words of every slot"""
    api = S.api
    cs = [S.ctxt(init_c[i]) for i in range(lm.NC)]
    ts = [S.trlwe(init_t[i]) for i in range(lm.NT)]
    for k, op in enumerate(prog):
        st = S.st[k % len(S.st)]
        kind = op["kind"]
        if kind == "nand":
            api.gNand(cs[op["out"]], cs[op["a"]], cs[op["b"]], st)
        elif kind == "user":
            api.gApply(user_op, cs[op["out"]], cs[op["a"]], st)
        elif kind == "copy":
            api.gCopy(cs[op["out"]], cs[op["a"]], st)
        elif kind == "lookup":
            nout = lm.DEFS[op["d"]][3]
            # the outputs in REQUEST order: one call per rising run of j (None: not requested), so a request 5, 0, 3 reaches the level's
            # list as the siblings 5, 0, 3 of one evaluation
            runs = [[op["outs"][0]]]
            for s, j in op["outs"][1:]:
                if j > runs[-1][-1][1]:
                    runs[-1].append((s, j))
                else:
                    runs.append([(s, j)])
            for run in runs:
                outs = [None] * nout
                for s, j in run:
                    outs[j] = cs[s]
                api.gLookup(outs, ts[op["table"]], cs[op["a"]], None if op["b"] is None else cs[op["b"]], lookups[op["d"]], st)
        elif kind == "spread":
            api.gSpread(ts[op["tout"]], ts[op["tin"]], op["stride"], op["reps"], st)
        elif kind == "lutrot":
            api.gLutRotate(ts[op["tout"]], ts[op["tin"]], cs[op["a"]], st, nout=op["nout"])
        else:
            api.gSampleExtractAndKeySwitch(cs[op["out"]], ts[op["tin"]], st, index=op["j"])
    for c in cs + ts:
        api.CtxtCopyD2H(c, S.st[0])
    api.Synchronize()
    return np.stack([c.tlwehost for c in cs]), np.stack([t.trlwehost for t in ts])


@pytest.mark.parametrize("two_lane", [0, 2])
@pytest.mark.parametrize("rename", [0, 1])
def test_random_dependent_programs(fresh, keys, rename, two_lane):
    """20 programs of about 40 ops over NAND, a user gate, lookups (nout 1, 2, 8; one and two operands), recorded Spread, LUT_ROTATE,
    SEIKS_AT and copies: every final value equals the model's, with and without renaming, level by level and on two lanes.  Every
    hazard class the generator plants occurs in every program."""
    progs, finals = program_references(keys)
    total = dict.fromkeys(lm.HAZARDS, 0)
    for _, _, prog in progs:
        for k, v in lm.hazards(prog).items():
            assert v >= 1, (k, v)
            total[k] += v
    print("hazards over the 20 programs:", total)
    S = Session(fresh, streams=2)
    api = S.api
    lookups = [api.DefineLookup(d[:2], d[2], d[3]) for d in lm.DEFS]
    user_op = api.define_gate((1, 0, 0), lm.USER_OFFSET, lm.user_tv())
    api.set_option("sched_rename", rename)
    api.set_option("sched_two_lane", two_lane)
    try:
        for i, ((init_c, init_t, prog), (want_c, want_t)) in enumerate(zip(progs, finals)):
            got_c, got_t = run_program(S, lookups, user_op, init_c, init_t, prog)
            assert np.array_equal(got_t, want_t), (i, "TRLWE", first_difference(got_t, want_t))
            assert np.array_equal(got_c, want_c), (i, "lvl0", first_difference(got_c, want_c))
    finally:
        api.set_option("sched_rename", 1)
        api.set_option("sched_two_lane", 1)
    S.close()


def test_end_to_end_under_genuine_keys(fresh, keys):
    """p = 4: a host-encrypted TRLWE holds four bit entries at coefficients m N / 4; a recorded Spread fills the boxes; the four padded
    addresses m / 8 are host-encrypted and read by recorded lookups; CtxtCopyD2H and ONE Synchronize.  Every read decrypts to its entry
    and every word equals the model's; a fifth lookup forms its address from two ciphertexts (1/8 + 2/8) by a (1, 1) definition."""
    S = Session(fresh)
    api = S.api
    st = S.st[0]
    table_words, addrs, v = lm.worked_example_inputs(keys)
    packed, table = api.Trlwe(), api.Trlwe()
    packed.trlwehost[:] = table_words
    api.CtxtCopyH2D(packed, st)
    api.gSpread(table, packed, 1, N // 4, st)
    one, two = api.DefineLookup((1, 0), 0, 1), api.DefineLookup((1, 1), 0, 1)
    ca, outs = [api.Ctxt(0) for _ in range(4)], [api.Ctxt(0) for _ in range(5)]
    for m in range(4):
        ca[m].tlwehost[:] = addrs[m]
        api.CtxtCopyH2D(ca[m], st)
        api.gLookup([outs[m]], table, ca[m], None, one, st)
    api.gLookup([outs[4]], table, ca[1], ca[2], two, st)
    for c in outs + [table]:
        api.CtxtCopyD2H(c, st)
    api.Synchronize()
    want_table = lm.spread(table_words, 1, N // 4)
    assert np.array_equal(table.trlwehost, want_table)
    for m in range(4):
        assert int(keys.decrypt(outs[m].tlwehost, 0)[0]) == int(v[m]), (m, list(v))
        assert np.array_equal(outs[m].tlwehost, lm.lookup(keys, (1, 0, 0, 1), want_table, addrs[m])[0]), m
    assert int(keys.decrypt(outs[4].tlwehost, 0)[0]) == int(v[3]), list(v)
    assert np.array_equal(outs[4].tlwehost, lm.lookup(keys, (1, 1, 0, 1), want_table, addrs[1], addrs[2])[0])
    S.close()


def test_refusals_and_the_ops_around_them(fresh, keys, data):
    """each -1 of the recorded entries with real handles: nothing is recorded (the scheduler's gate count stands still, the outputs
    keep their fill) and the ops recorded around the refusals give their words; "param_set" active; a handle of another set; no keys"""
    S = Session(fresh)
    api, lib = S.api, fresh.lib
    st = S.st[0]
    dev, raw = st.device_id(), st.st()
    tabs = [S.trlwe(data.tables[t]) for t in range(2)]
    a, b = S.ctxt(data.x[0]), S.ctxt(data.x[1])
    outs = [S.ctxt(None) for _ in range(8)]
    lvl1 = api.Ctxt(1)
    api.Synchronize()
    op1, op2, op8 = S.op("A", 1), S.op("B", 1), S.op("A", 8)

    def harr(cs):
        import ctypes
        return (ctypes.c_void_p * len(cs))(*[c._h for c in cs])

    def look(op=op1, nout=1, o=None, table=tabs[0], in0=a, in1=None):
        o = outs[:nout] if o is None else o
        return lib.cufhe_amd_enqueue_lookup(dev, raw, op, 0, nout, harr(o), table._h, in0._h, None if in1 is None else in1._h)

    def refused(rc, word):
        assert rc == -1 and word in lib.cufhe_amd_last_error(), (rc, lib.cufhe_amd_last_error())

    # a lookup recorded BEFORE the refusals, still pending while they are tried
    before = S.ctxt(None)
    api.Synchronize()
    api.sched_stats(reset=True)
    api.gLookup([before], tabs[0], a, None, op1, st)
    recorded = api.sched_stats().gates
    refused(look(op=op1 + 5), b"defined")                          # not a definition
    refused(look(op=api.LOOKUP_OP_BASE + api.MAX_LOOKUPS), b"defined")       # output 1 of definition 0: not an output-0 id
    refused(look(op=op8, nout=4), b"nout")
    refused(look(op=op1, nout=2), b"nout")
    refused(look(o=[lvl1]), b"level")
    refused(look(in0=lvl1), b"level")
    refused(look(table=a), b"level")
    refused(look(op=op2), b"second")                               # c1 != 0 without in1
    refused(look(op=op8, nout=8, o=outs[:7] + [outs[0]]), b"same")
    refused(look(op=op8, nout=8, o=outs[:7] + [a]), b"operand")    # nout > 1: an output is an operand
    refused(lib.cufhe_amd_enqueue_gate(dev, raw, op1, 0, outs[0]._h, a._h, None, None), b"unknown")
    sp = lib.cufhe_amd_enqueue_spread
    refused(sp(dev, raw, 0, tabs[0]._h, tabs[0]._h, 1, 4), b"must not be in")
    for stride, reps in ((3, 4), (1, 0), (0, 4), (2, 1024), (1, 2048), (-2, 4)):
        refused(sp(dev, raw, 0, tabs[1]._h, tabs[0]._h, stride, reps), b"powers of two")
    refused(sp(dev, raw, 0, a._h, tabs[0]._h, 1, 4), b"level 2")
    rt = lib.cufhe_amd_enqueue_lut_rotate
    refused(rt(dev, raw, 0, 1, tabs[0]._h, tabs[0]._h, a._h), b"must not be table")
    refused(rt(dev, raw, 0, 3, tabs[1]._h, tabs[0]._h, a._h), b"nout")
    refused(rt(dev, raw, 0, 1, tabs[1]._h, tabs[0]._h, tabs[0]._h), b"level 2")
    import ctypes
    ps = api.ps_index("default")
    api.ps_initialize(ps, keys.bk, keys.ksk)
    api.set_option("param_set", ps)
    try:
        for rc in (look(), sp(dev, raw, 0, tabs[1]._h, tabs[0]._h, 1, 4), rt(dev, raw, 0, 1, tabs[1]._h, tabs[0]._h, a._h)):
            assert rc == -1 and b"param_set" in lib.cufhe_amd_last_error()
        c2 = (ctypes.c_int32 * 2)(1, 0)
        opx = ctypes.c_int(-1)
        assert lib.cufhe_amd_define_lookup(c2, 0, 1, ctypes.byref(opx)) == -1 and b"param_set" in lib.cufhe_amd_last_error()
    finally:
        api.set_option("param_set", -1)
    # handles created under another set: a lvl0 ciphertext of "cggi16" has n = 500, a TRLWE of "k2n512" has (k + 1) N = 1536 words
    # (creating a handle needs no keys of the set)
    api.set_option("param_set", api.ps_index("cggi16"))
    try:
        other0 = api.Ctxt(0)
    finally:
        api.set_option("param_set", -1)
    api.set_option("param_set", api.ps_index("k2n512"))
    try:
        other2 = api.Trlwe()
    finally:
        api.set_option("param_set", -1)
    assert other0.tlwehost.size != n + 1 and other2.trlwehost.size != 2 * N
    word = b"another parameter set"
    refused(look(o=[other0]), word)                                # as an output,
    refused(look(in0=other0), word)                                # an address
    refused(look(op=op2, in1=other0), word)
    refused(look(table=other2), word)                              # and the table
    refused(sp(dev, raw, 0, other2._h, tabs[0]._h, 1, 4), word)
    refused(sp(dev, raw, 0, tabs[1]._h, other2._h, 1, 4), word)
    refused(rt(dev, raw, 0, 1, other2._h, tabs[0]._h, a._h), word)
    refused(rt(dev, raw, 0, 1, tabs[1]._h, other2._h, a._h), word)
    refused(rt(dev, raw, 0, 1, tabs[1]._h, tabs[0]._h, other0._h), word)
    # the N = 2048 ring: lookups write lvl0 ciphertexts of the gates' path and are refused; Spread and the rotation do not depend on it
    api.set_option("lvl0_ring", 2048)
    try:
        refused(look(), b"lvl0_ring")
    finally:
        api.set_option("lvl0_ring", 1024)
    # no output requested at all
    refused(lib.cufhe_amd_enqueue_lookup(dev, raw, op8, 0, 8, (ctypes.c_void_p * 8)(), tabs[0]._h, a._h, None), b"null")
    assert api.sched_stats().gates == recorded                     # nothing was recorded by any of them
    # a lookup recorded AFTER them, in place (nout = 1: the output may be the address operand)
    inplace = S.ctxt(data.x[0])
    api.gLookup([inplace], tabs[0], inplace, None, op1, st)
    for c in [before, inplace] + outs:
        api.CtxtCopyD2H(c, st)
    api.Synchronize()
    want = data.refs([(0, 0, "A", 1)])[(0, 0, "A", 1)][0]
    assert np.array_equal(before.tlwehost, want) and np.array_equal(inplace.tlwehost, want)
    assert all(np.all(c.tlwehost == FILL) for c in outs)
    # the definitions' own refusals, and the 65th
    import ctypes
    opx = ctypes.c_int(-1)
    dl = lib.cufhe_amd_define_lookup
    refused(dl((ctypes.c_int32 * 2)(0, 1), 0, 1, ctypes.byref(opx)), b"c0")
    for bad in (0, 3, 16, -1):
        refused(dl((ctypes.c_int32 * 2)(1, 0), 0, bad, ctypes.byref(opx)), b"nout")
    refused(dl(None, 0, 1, ctypes.byref(opx)), b"null")
    refused(dl((ctypes.c_int32 * 2)(1, 0), 0, 1, None), b"null")
    have = len(S.ops)
    for k in range(have, api.MAX_LOOKUPS):
        assert api.DefineLookup((1, 0), k, 1) == api.LOOKUP_OP_BASE + k
    refused(dl((ctypes.c_int32 * 2)(1, 0), 0, 1, ctypes.byref(opx)), b"full")
    # without keys: -3, and Spread needs none
    fresh.CleanUp()
    fresh.SetGPUNum(1)
    try:
        assert dl((ctypes.c_int32 * 2)(1, 0), 0, 1, ctypes.byref(opx)) == -3 and b"Initialize" in lib.cufhe_amd_last_error()
        t0, t1 = api.Trlwe(), api.Trlwe()
        t0.trlwehost[:] = data.tables[0]
        st2 = api.Stream()
        st2.Create()
        a2, o2 = api.Ctxt(0), api.Ctxt(0)
        assert lib.cufhe_amd_enqueue_lut_rotate(st2.device_id(), st2.st(), 0, 1, t1._h, t0._h, a2._h) == -3
        api.CtxtCopyH2D(t0, st2)
        api.gSpread(t1, t0, 4, 64, st2)
        api.CtxtCopyD2H(t1, st2)
        api.Synchronize()
        assert np.array_equal(t1.trlwehost, lc.spread(data.tables[0], 4, 64))
        st2.Destroy()
    finally:
        fresh.Initialize(keys.bk, keys.ksk)
    # ids count from the last CleanUp again
    assert api.DefineLookup((1, 0), 0, 1) == api.LOOKUP_OP_BASE


def build_cpp_program():
    """tests/cpp/test_recorded_lut.cpp -> tests/cpp/test_recorded_lut, with the flags tests/cpp_build.py gives the other C++ programs"""
    import cpp_build
    cdefs, libs = cpp_build.hip_flags()
    root = ol.ROOT
    exe = os.path.join(root, "tests", "cpp", "test_recorded_lut")
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + cdefs +
                          ["-o", exe, os.path.join(root, "tests", "cpp", "test_recorded_lut.cpp"),
                           "-L" + os.path.join(root, "cufhe_amd"), "-lcufhe_amd", "-L" + os.path.join(root, "oracle"), "-loracle",
                           "-Wl,-rpath," + os.path.join(root, "cufhe_amd"), "-Wl,-rpath," + os.path.join(root, "oracle")] + libs)
    return exe


def test_cpp_recorded_lut(engine, keys):
    """tests/cpp/test_recorded_lut.cpp: the worked example through DefineLookup / gSpread / gLookup of include/cufhe_amd.hpp"""
    exe = build_cpp_program()
    engine.CleanUp()                      # the C++ program owns the device state while it runs
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        engine.SetGPUNum(1)
        engine.Initialize(keys.bk, keys.ksk)
