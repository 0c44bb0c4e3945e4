"""Random programs over every kind of record the per-gate API makes, with the in-order model they are checked against.

A program is a list of records (plain tuples, made without a device by `generate`): built-in gates, user gates of one to three
operands, multi-output evaluations recorded together (ApplyMulti) or sibling by sibling (Apply with user_op_output), the TRLWE-level
operations, SEIKS_AT, CMUXNTT, in-place CMUXRotateNTT chains, circuit bootstraps into TRGSW holders, TRGSW2NTT, explicit copies,
StreamQuery polls, Flush, and Synchronize followed by host edits -- in copying and device-resident forms.

`Model` walks the records in issue order with the reference's semantics, as the random test of tests/test_gpu_scheduler.py encodes
them: every ciphertext has a host value and a device value; a copying record uploads its operands' host values and delivers its
result to both members of the output, a g-record touches device values only.  Values are ids of nodes of a DAG (record, operands),
evaluated afterwards on the CPU with the checkers the suite already trusts (`evaluate`), on threads, once per distinct
(operation, operand values).  The model also counts the hazard classes the program contains (`Model.hazards`): the generator is
only worth something while every class a mode can express occurs, which tests/test_program_model.py asserts for the committed seeds.

`issue` plays a program through cufhe_amd.api and records what the host could observe: every host member after Synchronize, the
members delivered through a stream after a StreamQuery that returned true, and everything at the end.
"""
from concurrent.futures import ThreadPoolExecutor
import os

import numpy as np

import lvl2_multi_checker as mc2
import lvl2_user_gate_checker as lc
import multi_output_checker as mc
import oracle_lib as ol
import packed_rom_checker as pr
import user_gate_checker as uc

N, n = ol.N, ol.n
TWO = ["NAND", "NOR", "XNOR", "AND", "OR", "XOR", "ANDNY", "ANDYN", "ORNY", "ORYN"]
TRGSW_WORDS = uc.STEP_WORDS
LEVEL_WORDS = {0: n + 1, 1: N + 1, 2: 2 * N}
POOLS = {"a": {0: 10, 1: 5, 2: 5, 3: 3}, "b": {0: 26, 1: 0, 2: 0, 3: 0}, "c": {0: 14, 1: 0, 2: 0, 3: 0}, "d": {0: 12, 1: 5, 2: 3, 3: 2}}
STREAMS = {"a": 5, "b": 4, "c": 3, "d": 4}
SEEDS = {"a": (0, 1, 2), "b": (0, 1), "c": (0, 1, 2), "d": (0, 1, 2)}      # the committed programs of each mode (CUFHE_AMD_STRESS_SEEDS multiplies them)


def seeds(mode):
    k = int(os.environ.get("CUFHE_AMD_STRESS_SEEDS", "1"))
    base = SEEDS[mode]
    return [s + 100 * r for r in range(k) for s in base]


def user_defs():
    """the user gates every program may use: (coeffs, offset, test vector, nout); single-output ones of arity 1, 2, 3 first, then
    multi-output ones of 2, 4 and 8 outputs"""
    rng = np.random.default_rng(2200)
    defs = []
    for i, nout in enumerate((1, 1, 1, 2, 4, 8)):
        arity = 1 + i % 3
        c = [int(rng.integers(1, 4)) * (1 if rng.integers(0, 2) else -1)] + [int(rng.integers(-3, 4)) or 1 for _ in range(arity - 1)]
        tv = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
        defs.append((tuple(c + [0] * (3 - arity)), int(rng.integers(0, 1 << 32)), tv, nout))
    return defs


def arity_of(d):
    return 3 - [c == 0 for c in d[0]][::-1].index(False) if any(d[0]) else 1


SINGLE, MULTI = (0, 1, 2), (3, 4, 5)


def user_defs_ring():
    """mode (c), the N = 2048 ring: the same six shapes with test vectors of 2048 64-bit torus words (cufhe_amd_lvl2_define_gate)"""
    rng = np.random.default_rng(2201)
    return [(c, off, rng.integers(0, 2**64, ol.N2, dtype=np.uint64), nout) for c, off, _, nout in user_defs()]


def user_defs_set(ring_n):
    """mode (d), a compiled parameter set whose ring has ring_n coefficients (cufhe_amd_ps_define_gate)"""
    rng = np.random.default_rng(2202)
    return [(c, off, rng.integers(0, 1 << 32, size=ring_n, dtype=np.uint64).astype(np.uint32), nout) for c, off, _, nout in user_defs()]


class Env:
    """what a mode other than the default ring changes: the definitions, the op id of a sibling output, the checkers behind `evaluate`
    and the word counts.  kind "ring": keys2 = oracle_lib.KeysLvl2 (lvl2_user_gate_checker, lvl2_multi_checker); kind "set": checker =
    ps_user_gate_checker.Checker of the set (its oracle for everything else), TRGSW words = steps of its bootstrapping key."""

    def __init__(self, kind, keys2=None, checker=None):
        self.kind, self.keys2, self.C = kind, keys2, checker
        if kind == "ring":
            self.defs, self.level_words = user_defs_ring(), dict(LEVEL_WORDS)
        else:
            self.defs = user_defs_set(checker.N)
            self.level_words = {0: checker.words[0], 1: checker.words[1], 2: checker.acc_words}

    def trgsw(self, i):
        C = self.C
        return np.ascontiguousarray(C.K.bk[i * C.step_words:(i + 1) * C.step_words])

# hazard classes; the last one needs renaming ("sched_rename" 1) to be expressible
CLASSES_A = ["raw_gate_to_tl_bootstrap", "raw_seiks_at_to_gate", "raw_seiks_at_to_user_gate", "raw_circuit_bootstrap_to_selector",
             "raw_cmux_to_seiks_at", "war_trlwe_after_cmux", "war_holder_upload_after_cmux", "war_holder_circuit_bootstrap_after_cmux",
             "waw_level0", "waw_level1", "waw_level2", "waw_level3", "cmux_rotate_chain_of_3_in_place", "cmux_in_place_on_c1",
             "cmux_in_place_on_c0", "holder_host_rewritten_under_copying_cmux", "siblings_adjacent", "siblings_separated_by_operand_write",
             "siblings_separated_by_flush", "siblings_on_different_streams", "group_outputs_all_have_readers",
             "kind2_lvl0_output_fetched_and_polled_on_another_stream", "kinds_0_1_2_and_circuit_bootstrap_between_two_flushes"]
CLASSES_B = ["waw_level0", "group_outputs_all_have_readers", "war_level0_gate_output_after_readers", "in_place_gate"]
CLASSES_C = ["siblings_adjacent", "siblings_separated_by_operand_write", "siblings_separated_by_flush", "siblings_on_different_streams",
             "waw_level0", "war_level0_gate_output_after_readers", "in_place_gate"]
CLASSES_D = ["raw_gate_to_tl_bootstrap", "raw_cmux_to_seiks_at", "war_trlwe_after_cmux", "war_holder_upload_after_cmux",
             "waw_level0", "waw_level1", "waw_level2", "waw_level3", "cmux_in_place_on_c1", "cmux_in_place_on_c0",
             "holder_host_rewritten_under_copying_cmux", "siblings_adjacent", "siblings_separated_by_operand_write",
             "siblings_separated_by_flush", "siblings_on_different_streams", "war_level0_gate_output_after_readers", "in_place_gate"]


class Model:
    def __init__(self, pools, rng, level_words=None):
        self.level_words = level_words or LEVEL_WORDS
        self.nodes = []            # vid -> (kind, params, operand vids, record index)
        self.memo = {}
        self.records = []
        self.host, self.dev = {}, {}
        self.track = {}            # name -> dict: what wrote the device value (while on record), who read it
        self.hk = {}               # name -> (kind of the record whose result travels to the host member, its stream, fetched by D2H)
        self.host_stream = {}      # name -> stream of the newest delivery to the host member
        self.copying_cmux_named = set()
        self.hazards = {}
        self.window = set()        # kinds recorded since the last Flush / Synchronize
        self.names = []
        for level, count in pools.items():
            for i in range(count):
                name = (level, i)
                self.names.append(name)
                self.dev[name] = None
                self.host[name] = None if level == 3 else self.const(rng.integers(0, 1 << 32, size=self.level_words[level], dtype=np.uint64).astype(np.uint32))
                self.track[name] = self._fresh()

    @staticmethod
    def _fresh():
        return {"w": None, "on": False, "read": False, "cmux_read": False, "rot": 0, "st": None}

    def count(self, cls):
        self.hazards[cls] = self.hazards.get(cls, 0) + 1

    def const(self, words):
        self.nodes.append(("const", words, (), len(self.records) - 1))
        return len(self.nodes) - 1

    def node(self, kind, params, operands):
        key = (kind, params, tuple(operands))
        if key not in self.memo:
            self.nodes.append((kind, params, tuple(operands), len(self.records) - 1))
            self.memo[key] = len(self.nodes) - 1
        return self.memo[key]

    def snapshot(self, names=None):
        return {x: self.host[x] for x in (names if names is not None else self.names) if self.host[x] is not None}

    # ---- one record ----
    def apply(self, rec):
        self.records.append(rec)
        kind = rec[0]
        if kind in ("gate", "user", "sib", "boot", "refresh", "seiks_at", "cmux", "cmuxrot", "cb"):
            self._op(rec)
        elif kind == "multi":
            _, d, copying, outs, ins, st = rec
            if all(self.track[o]["read"] for o in outs):
                self.count("group_outputs_all_have_readers")
            ev = None
            for j, o in enumerate(outs):
                ev = self._op(("sib", d, j, copying, o, ins, st), ev)
        elif kind == "ntt":
            _, h, words, st = rec
            if h in self.copying_cmux_named:
                self.count("holder_host_rewritten_under_copying_cmux")
                self.copying_cmux_named.discard(h)
            self.host[h] = self.node("trgsw", len(self.records) - 1, ())
            self.hk.pop(h, None)
            self._upload(h, st, explicit=True)
        elif kind == "h2d":
            self._upload(rec[1], rec[2], explicit=True)
        elif kind == "d2h":
            _, x, st = rec
            t = self.track[x]
            t["read"] = True
            self.host[x] = self.dev[x]
            self.host_stream[x] = st
            self.hk[x] = (t["w"] if t["on"] else None, t["st"], True)
        elif kind in ("poll", "wait"):          # StreamQuery(st) once / until it returns true: what was delivered through st may be looked at
            rec_names = [x for x in self.names if self.host_stream.get(x) == rec[1]]
            self.records[-1] = rec = (kind, rec[1], self.snapshot(rec_names))
            if kind == "wait":
                for x in rec[2]:
                    w, wst, by_d2h = self.hk.get(x, (None, None, False))
                    if w in ("seiks", "seiks_at") and by_d2h and wst != rec[1]:
                        self.count("kind2_lvl0_output_fetched_and_polled_on_another_stream")
        elif kind == "flush":
            self.window = set()
        elif kind == "sync":
            self.records[-1] = ("sync", self.snapshot())
            for x in self.names:
                self.track[x] = self._fresh()
            self.hk, self.copying_cmux_named, self.window = {}, set(), set()
        elif kind == "edit":
            _, x, words = rec
            self.host[x] = self.const(words)
        else:
            raise ValueError(kind)

    def _upload(self, x, st, explicit):
        t = self.track[x]
        if explicit:
            if t["on"]:
                self.count("waw_level%d" % x[0])
            if x[0] == 2 and t["cmux_read"]:
                self.count("war_trlwe_after_cmux")
            if x[0] == 3 and t["cmux_read"]:
                self.count("war_holder_upload_after_cmux")
            t.update(read=False, cmux_read=False)
        t.update(w="upload", on=True, rot=0, st=st)
        self.dev[x] = self.host[x]

    def _op(self, rec, ev=None):
        kind = rec[0]
        if kind == "gate":
            _, name, copying, out, ins, st = rec
            wk, level_kind = "gate", out[0]
        elif kind == "user":
            _, d, copying, out, ins, st = rec
            wk, level_kind = "user", out[0]
        elif kind == "sib":
            _, d, j, copying, out, ins, st = rec
            wk, level_kind = "user", out[0]
        elif kind in ("boot", "refresh", "cb"):
            _, copying, out, x, st = rec
            ins, wk, level_kind = (x,), kind, 2
        elif kind == "seiks_at":
            _, j, copying, out, x, st = rec
            ins, wk, level_kind = (x,), "seiks_at" if j else "seiks", 2
        elif kind == "cmux":
            _, copying, out, cs, c1, c0, st = rec
            ins, wk, level_kind = (c1, c0, cs), "cmux", 2
        else:
            _, e, copying, out, cs, c, st = rec
            ins, wk, level_kind = (c, cs), "rot", 2
        cmux = kind in ("cmux", "cmuxrot")
        sk = [(self.hk.get(x, (None,))[0] if copying else (self.track[x]["w"] if self.track[x]["on"] else None)) for x in ins]
        if kind == "boot" and sk[0] in ("gate", "user"):
            self.count("raw_gate_to_tl_bootstrap")
        if kind in ("gate", "user", "sib") and "seiks_at" in sk:
            self.count("raw_seiks_at_to_gate" if kind == "gate" else "raw_seiks_at_to_user_gate")
        if cmux and sk[-1] == "cb":
            self.count("raw_circuit_bootstrap_to_selector")
        if kind == "seiks_at" and sk[0] == "cmux":
            self.count("raw_cmux_to_seiks_at")
        to = self.track[out]
        if to["on"]:
            self.count("waw_level%d" % out[0])
        if out[0] == 2 and to["cmux_read"]:
            self.count("war_trlwe_after_cmux")
        if out[0] == 3 and to["cmux_read"]:
            self.count("war_holder_circuit_bootstrap_after_cmux")
        if out[0] <= 1 and to["read"] and out not in ins:
            self.count("war_level0_gate_output_after_readers" if out[0] == 0 else "war_level1_gate_output_after_readers")
        if out[0] <= 1 and out in ins:
            self.count("in_place_gate")
        if kind == "cmux" and out == ins[0]:
            self.count("cmux_in_place_on_c1")
        if kind == "cmux" and out == ins[1] and out != ins[0]:
            self.count("cmux_in_place_on_c0")
        chain = 0
        if kind == "cmuxrot" and out == ins[0]:
            chain = to["rot"] + 1 if to["on"] and to["w"] == "rot" else 1
            if chain == 3:
                self.count("cmux_rotate_chain_of_3_in_place")
        for x in ins:
            if copying:
                self._upload(x, st, explicit=False)
            self.track[x]["read"] = True
            if cmux:
                self.track[x]["cmux_read"] = True
        if cmux and copying:
            self.copying_cmux_named.add(ins[-1])
        to.update(w=wk, on=True, read=False, cmux_read=False, rot=chain, st=st)
        self.window.add("cb" if kind == "cb" else 2 if level_kind == 2 else out[0])
        if self.window >= {0, 1, 2, "cb"} and "done" not in self.window:
            self.count("kinds_0_1_2_and_circuit_bootstrap_between_two_flushes")
            self.window.add("done")
        # the value
        ops = [self.dev[x] for x in ins]
        assert all(v is not None for v in ops), rec
        if kind == "gate":
            v = self.node("gate", (rec[1], out[0]), ops)
        elif kind == "user":
            v = self.node("user", (rec[1], out[0]), ops)
        elif kind == "sib":
            ev = ev if ev is not None else self.node("multi", (rec[1], out[0]), ops)
            v = self.node("output", rec[2], (ev,))
        elif kind == "seiks_at":
            v = self.node("seiks_at", rec[1], ops)
        elif kind == "cmuxrot":
            v = self.node("cmuxrot", rec[1], ops)
        else:
            v = self.node(kind, None, ops)
        self.dev[out] = v
        if copying:
            self.host[out] = v
            self.host_stream[out] = st
            self.hk[out] = (wk, st, False)
        return ev


# ---- generation ----
def generate(mode, seed, level_words=None):
    """the records of program `seed` of mode "a" (the default ring, every kind), "b" (the netlist form: device-resident lvl0 gates,
    user gates and multi-output evaluations, every value fetched at the end), "c" (the N = 2048 ring: built-in gates, lvl2 user gates
    and siblings recorded one by one) or "d" (a compiled parameter set, whose word counts are level_words: the records do not depend
    on them); returns the Model that walked them (records, hazards)"""
    if mode in ("c", "d"):
        rng = np.random.default_rng(2200 + 17 * seed + (9000 if mode == "c" else 13000))
        data = np.random.default_rng(77000 + seed)              # the words come from a generator of their own
        m = Model(POOLS[mode], data, level_words)
        if mode == "c":
            _generate_c(m, rng, data, seed)
        else:
            _generate_a(m, rng, 60, "d", data)
        for x in m.names:
            if m.dev[x] is not None and m.dev[x] != m.host[x]:
                m.apply(("d2h", x, int(rng.integers(STREAMS[mode]))))
        m.apply(("sync",))
        return m
    rng = np.random.default_rng(2200 + 17 * seed + (0 if mode == "a" else 5000))
    m = Model(POOLS[mode], rng)
    if mode == "a":
        _generate_a(m, rng)
        for x in m.names:            # every holder a circuit bootstrap wrote on the device, and half of the other device values, are fetched
            if m.dev[x] is not None and m.dev[x] != m.host[x] and (m.nodes[m.dev[x]][0] == "cb" or rng.random() < 0.5):
                m.apply(("d2h", x, int(rng.integers(STREAMS["a"]))))
    else:
        _generate_b(m, rng)
    m.apply(("sync",))
    return m


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _generate_a(m, rng, records=120, mode="a", data=None):
    """mode "d" (a parameter set) leaves out what the sets refuse: circuit bootstraps, the rotating CMUX, SEIKS_AT at an index other than
    0 and ApplyMulti (a set's siblings are recorded one by one); its TRGSW words are steps of the set's bootstrapping key, by index"""
    defs = user_defs()
    pool = {lvl: [(lvl, i) for i in range(c)] for lvl, c in POOLS[mode].items()}
    sts = list(range(STREAMS[mode]))
    on_set = mode == "d"
    data = data if data is not None else rng

    def trgsw_words():
        return int(rng.integers(64)) if on_set else rng.integers(0, 1 << 32, size=TRGSW_WORDS, dtype=np.uint64).astype(np.uint32)

    last = {}                   # kind -> newest output of that kind of record
    rot = None                  # (trlwe, holder) of the in-place rotation chain in progress
    sib = None                  # the one-by-one evaluation in progress

    def ready(x, copying):
        return (m.host[x] if copying else m.dev[x]) is not None

    def some(level, copying, prefer=None):
        if prefer is not None and prefer[0] == level and ready(prefer, copying) and rng.random() < 0.6:
            return prefer
        c = [x for x in pool[level] if ready(x, copying)]
        return _pick(rng, c) if c else None

    # the holders are filled by TRGSW2NTT first
    for h in pool[3]:
        m.apply(("ntt", h, trgsw_words(), _pick(rng, sts)))
    # two packed-ROM reads in small, so that no seed misses them: a gate's result bootstrapped to a TRLWE and circuit-bootstrapped to a
    # selector, then three rotating CMUX steps in place on that TRLWE -- each on a stream of its own
    for k in range(0 if on_set else 2):
        g, t, h = pool[0][9 - k], pool[2][k], pool[3][k]
        m.apply(("gate", _pick(rng, TWO), True, g, (_pick(rng, pool[0]), _pick(rng, pool[0])), _pick(rng, sts)))
        m.apply(("boot", False, t, g, _pick(rng, sts)))
        m.apply(("cb", False, h, g, _pick(rng, sts)))
        for _ in range(3):
            m.apply(("cmuxrot", int(_pick(rng, pr.EXPONENTS)), False, t, h, t, _pick(rng, sts)))
        rot = (t, h)
    if on_set:
        # the crossings between kinds that 60 drawn records may miss, once per program with drawn operands and streams: gates bootstrapped
        # to TRLWEs, CMUXNTT in place on c1 and on c0, its result extracted, a holder re-filled under a copying CMUXNTT that named its host
        # words, a TRLWE overwritten after a CMUXNTT read it, two lvl1 gates into one output, siblings with a Flush between them
        g0, g1, (t0, t1, t2), (h0, h1) = pool[0][11], pool[0][10], pool[2], pool[3]
        s_ = lambda: _pick(rng, sts)  # noqa: E731
        m.apply(("gate", _pick(rng, TWO), True, g0, (_pick(rng, pool[0][:6]), _pick(rng, pool[0][:6])), s_()))
        m.apply(("user", int(_pick(rng, SINGLE[:1])), True, g1, (g0,), s_()))
        m.apply(("boot", False, t0, g0, s_()))
        m.apply(("boot", True, t1, g1, s_()))
        m.apply(("cmux", False, t0, h0, t0, t1, s_()))
        m.apply(("cmux", False, t1, h1, t0, t1, s_()))
        m.apply(("seiks_at", 0, False, pool[0][9], t1, s_()))
        m.apply(("cmux", True, t2, h0, t0, t1, s_()))
        m.apply(("ntt", h0, trgsw_words(), s_()))
        m.apply(("boot", False, t0, g1, s_()))
        m.apply(("gate", _pick(rng, TWO), True, pool[1][0], (pool[1][1], pool[1][2]), s_()))
        m.apply(("gate", "MUX", False, pool[1][0], (pool[1][0], pool[1][1], pool[1][2]), s_()))
        pair = (pool[0][7], pool[0][8])
        m.apply(("sib", 3, 1, True, pair[1], (g0,), s_()))
        m.apply(("flush",))
        m.count("siblings_separated_by_flush")
        m.apply(("sib", 3, 0, True, pair[0], (g0,), s_()))
    while len(m.records) < records:
        st = _pick(rng, sts)
        copying = bool(rng.random() < 0.45)
        if sib is not None:
            u = rng.random()
            if u < 0.45:
                d, cp, outs, ins, order, st0 = sib
                j = order.pop()
                st1 = _pick(rng, sts) if rng.random() < 0.5 else st0
                if sib_state["n"]:
                    m.count("siblings_separated_by_operand_write" if sib_state["write"] else "siblings_separated_by_flush" if sib_state["flush"]
                            else "siblings_adjacent" if not sib_state["other"] else "siblings_separated_by_other_records")
                    if st1 != st0:
                        m.count("siblings_on_different_streams")
                m.apply(("sib", d, j, cp, outs[j], ins, st1))
                sib_state.update(n=sib_state["n"] + 1, write=False, flush=False, other=False)
                if not order:
                    sib = None
                continue
            if u < 0.65:
                d, cp, outs, ins, order, st0 = sib
                a = [x for x in pool[ins[0][0]] if ready(x, cp) and x not in outs]
                if a:
                    m.apply(("gate", _pick(rng, TWO), cp, ins[0], (_pick(rng, a), _pick(rng, a)), st0))
                    sib_state["write"] = True
                continue
            if u < 0.73:
                m.apply(("flush",))
                sib_state["flush"] = True
                continue
            sib_state["other"] = True
        r = rng.random()
        level = 1 if rng.random() < 0.3 else 0
        if r < 0.12:                                   # built-in gate, sometimes on the newest SEIKS_AT result, sometimes in place
            a = some(level, copying, last.get("seiks_at"))
            b, c = some(level, copying), some(level, copying)
            if a is None or b is None:
                continue
            out = a if rng.random() < 0.2 else _pick(rng, pool[level])
            q = rng.random()
            if q < 0.1:
                m.apply(("gate", "NOT", copying, out, (a,), st))
            elif q < 0.25:
                m.apply(("gate", "MUX", copying, out, (a, b, c), st))
            else:
                m.apply(("gate", _pick(rng, TWO), copying, out, (a, b), st))
            last["gate"] = out
        elif r < 0.20:                                 # user gate of arity 1, 2 or 3
            d = int(_pick(rng, SINGLE))
            ins = [some(level, copying, last.get("seiks_at"))] + [some(level, copying) for _ in range(arity_of(defs[d]) - 1)]
            if None in ins:
                continue
            out = _pick(rng, pool[level])
            m.apply(("user", d, copying, out, tuple(ins), st))
            last["gate"] = out
        elif r < 0.38:                                 # multi-output evaluation: together, or sibling by sibling
            d = int(_pick(rng, MULTI))
            if on_set and rng.random() < 0.6:          # (eight siblings at a time would fill a program of 60 records)
                continue
            nout = defs[d][3]
            if nout > len(pool[level]) - 3:
                level = 0
            ins = tuple(some(level, copying) for _ in range(arity_of(defs[d])))
            if None in ins:
                continue
            free = [x for x in pool[level] if x not in ins]
            if len(free) < nout:
                continue
            free.sort(key=lambda x: (not m.track[x]["read"], rng.random()))       # outputs whose values have recorded readers first
            outs = tuple(free[:nout])
            if nout <= 4 and all(ready(o, copying) for o in outs) and rng.random() < 0.7:      # every output's present value gets a recorded reader first
                for q in range(0, nout, 2):
                    m.apply(("gate", _pick(rng, TWO), copying, _pick(rng, [x for x in free[nout:]] or [ins[0]]), (outs[q], outs[q + 1]), _pick(rng, sts)))
            if on_set and sib is not None:
                continue
            if sib is None and (on_set or rng.random() < 0.65):
                order = [int(j) for j in rng.permutation(nout)]
                sib = (d, copying, outs, ins, order, st)
                sib_state = {"n": 0, "write": False, "flush": False, "other": False}
            else:
                m.apply(("multi", d, copying, outs, ins, st))
        elif r < 0.42:                                 # TL_BOOTSTRAP of what a gate produced, Refresh
            if rng.random() < 0.7:
                x = some(0, copying, last.get("gate"))
                if x is not None:
                    m.apply(("boot", copying, _pick(rng, pool[2]), x, st))
            else:
                x = some(2, copying)
                if x is not None:
                    m.apply(("refresh", copying, x if rng.random() < 0.3 else _pick(rng, pool[2]), x, st))
        elif r < 0.52:                                 # SEIKS_AT(j), often fetched on another stream and polled there
            x = some(2, copying, last.get("cmux"))
            if x is None:
                continue
            out = _pick(rng, pool[0])
            m.apply(("seiks_at", int(_pick(rng, (0,) if on_set else (0, 1, 63, 64, 511, 1023))), copying, out, x, st))
            last["seiks_at"] = out
            if rng.random() < 0.6:
                st2 = _pick(rng, [s for s in sts if s != st])
                m.apply(("d2h", out, st2))
                m.apply(("wait", st2))
        elif r < 0.63:                                 # CMUXNTT, now and then in place on c1 or on c0
            cs = some(3, copying, last.get("cb"))
            c1, c0 = some(2, copying), some(2, copying)
            if None in (cs, c1, c0):
                continue
            q = rng.random()
            res = c1 if q < 0.25 else c0 if q < 0.5 else _pick(rng, pool[2])
            m.apply(("cmux", copying, res, cs, c1, c0, st))
            last["cmux"] = res
        elif r < 0.75:                                 # CMUXRotateNTT: in place, going on with the chain of the step before
            if on_set:
                continue
            if rot is not None and ready(rot[0], False) and ready(rot[1], False) and rng.random() < 0.92:
                c, cs, cp = rot[0], rot[1], False
            else:
                c, cs, cp = some(2, copying), some(3, copying, last.get("cb")), copying
            if c is None or cs is None:
                continue
            res = c if rng.random() < 0.85 else _pick(rng, pool[2])
            m.apply(("cmuxrot", int(_pick(rng, pr.EXPONENTS)), cp, res, cs, c, st))
            rot = (res, cs)
        elif r < 0.81:                                 # circuit bootstrap of a lvl0 value the program produced
            x = some(0, copying, last.get("gate"))
            if x is None or on_set:
                continue
            out = _pick(rng, pool[3])
            m.apply(("cb", copying, out, x, st))
            last["cb"] = out
        elif r < 0.85:                                 # a holder re-filled by TRGSW2NTT mid-program
            named = sorted(m.copying_cmux_named)
            m.apply(("ntt", _pick(rng, named) if named else _pick(rng, pool[3]), trgsw_words(), st))
        elif r < 0.89:
            x = some(int(_pick(rng, (0, 0, 1, 2, 3))), True)
            if x is not None:
                m.apply(("h2d", x, st))
        elif r < 0.93:
            x = some(int(_pick(rng, (0, 0, 1, 2, 3))), False)
            if x is not None:
                m.apply(("d2h", x, st))
        elif r < 0.96:
            m.apply(("poll", st))
        elif r < 0.98:
            m.apply(("flush",))
        elif sib is None:                              # Synchronize, then the host edits a few ciphertexts
            m.apply(("sync",))
            rot = None
            last.clear()
            for _ in range(2):
                x = _pick(rng, pool[int(_pick(rng, (0, 1, 2)))])
                m.apply(("edit", x, data.integers(0, 1 << 32, size=m.level_words[x[0]], dtype=np.uint64).astype(np.uint32)))


def _generate_c(m, rng, data, seed):
    """The N = 2048 ring ("lvl0_ring" 2048), lvl0 ciphertexts only, about 30 records: the eight outputs of one evaluation recorded one
    by one in shuffled order (copying) -- with nothing, a write to an operand, or a Flush between two of them, on changing streams --,
    then four outputs of the same definition on the same operands again, device-resident, into ciphertexts that hold siblings of the
    first; a single-output user gate; built-in gates in place and over values that still have readers.  Scripted rather than drawn: an
    evaluation costs the ring's Python checker seconds and threads do not help it, so a program holds as few as the hazard classes
    allow: the operand is written once (two evaluations), the second round of siblings adds none (same definition, same operand
    values), and the single-output user gate is in the first seed only."""
    pool = [(0, i) for i in range(POOLS["c"][0])]
    ins, outs, extra = tuple(pool[0:3]), pool[3:11], pool[11:14]
    sts = list(range(STREAMS["c"]))
    m.apply(("gate", _pick(rng, TWO), True, extra[0], (ins[0], ins[1]), sts[0]))
    if seed % 3 == 0:
        m.apply(("user", 1, True, extra[1], (extra[0], ins[1]), sts[1]))
    state = {"st": sts[0], "k": 0}

    def sibling(j, copying, out, gap):
        if gap == "write":
            m.apply(("gate", _pick(rng, TWO), True, ins[0], (ins[1], ins[2]), state["st"]))
        elif gap == "flush":
            m.apply(("flush",))
        if gap:
            m.count("siblings_adjacent" if gap == "adjacent" else "siblings_separated_by_operand_write" if gap == "write" else "siblings_separated_by_flush")
            state["k"] += 1
            if state["k"] % 2:
                state["st"] = sts[(sts.index(state["st"]) + 1) % len(sts)]
                m.count("siblings_on_different_streams")
        m.apply(("sib", 5, j, copying, out, ins, state["st"]))

    gaps = ["adjacent", "flush", "write", "adjacent", "flush", "adjacent", "flush"]
    for k, j in enumerate(int(j) for j in rng.permutation(8)):
        sibling(j, True, outs[j], gaps[(k - 1 + 2 * seed) % 7] if k else None)
    m.apply(("gate", _pick(rng, TWO), True, extra[2], (outs[0], outs[1]), sts[2]))              # readers of two sibling outputs ...
    m.apply(("gate", "MUX", False, outs[2], (outs[2], outs[3], outs[4]), sts[1]))               # ... and a gate in place on a third
    for k, j in enumerate(int(j) for j in rng.permutation(8)[:4]):                              # the same evaluation again, device-resident
        sibling(j, False, outs[k], (None, "flush", "adjacent", "adjacent")[k])
    m.apply(("gate", _pick(rng, TWO), False, extra[2], (extra[2], outs[7]), sts[0]))
    m.apply(("gate", "NOT", False, outs[6], (outs[6],), sts[1]))


def _generate_b(m, rng, phase1=68, phase2=12):
    """phase 1: built-in and single-output user gates only (a flush that compile_two_lane can take); Synchronize; phase 2 adds
    multi-output evaluations, whose flush stays in the level order (shares_rotation)"""
    defs = user_defs()
    pool = [(0, i) for i in range(POOLS["b"][0])]
    n_in = 10
    sts = list(range(STREAMS["b"]))
    for i in range(n_in):
        m.apply(("h2d", pool[i], sts[i % len(sts)]))
    last = pool[0]

    def defined():
        return [x for x in pool if m.dev[x] is not None]

    def one(multi_ok):
        nonlocal last
        st = _pick(rng, sts)
        d_ = defined()
        a = last if rng.random() < 0.5 else _pick(rng, d_)
        b, c = _pick(rng, d_), _pick(rng, d_)
        o = a if rng.random() < 0.15 else _pick(rng, pool[n_in:])
        r = rng.random()
        if multi_ok and r < 0.5:
            d = int(_pick(rng, MULTI))
            ins = (a, b, c)[:arity_of(defs[d])]
            free = [x for x in pool[n_in:] if x not in ins]
            free.sort(key=lambda x: (not m.track[x]["read"], rng.random()))
            outs = tuple(free[:defs[d][3]])
            m.apply(("multi", d, False, outs, ins, st))
            last = outs[0]
            return
        if r < 0.05:
            m.apply(("gate", "NOT", False, o, (a,), st))
        elif r < 0.15:
            m.apply(("gate", "MUX", False, o, (a, b, c), st))
        elif r < 0.27:
            d = int(_pick(rng, SINGLE))
            m.apply(("user", d, False, o, (a, b, c)[:arity_of(defs[d])], st))
        else:
            m.apply(("gate", _pick(rng, TWO), False, o, (a, b), st))
        last = o

    for _ in range(phase1):
        one(False)
    for i, x in enumerate(pool):
        if m.dev[x] is not None:
            m.apply(("d2h", x, sts[i % len(sts)]))
    m.apply(("sync",))
    for _ in range(phase2):
        one(True)
    for i, x in enumerate(pool):
        if m.dev[x] is not None:
            m.apply(("d2h", x, sts[i % len(sts)]))


# ---- evaluation ----
def evaluate(m, vids, keys, cb_oracle=None, threads=16, env=None):
    """the words of the values `vids` (and of everything they depend on): {vid: words}; a TRGSW value is the pair (torus words, None) --
    its NTT image is what the library made of it (TRGSW2NTT) or what `cb_oracle(list of lvl0 words) -> [(torus, ntt)]` returns"""
    defs = env.defs if env else user_defs()
    need, stack = set(), list(vids)
    while stack:
        v = stack.pop()
        if v not in need:
            need.add(v)
            stack.extend(m.nodes[v][2])
    depth = {}
    for v in sorted(need):                              # operands have smaller ids
        depth[v] = 1 + max((depth[o] for o in m.nodes[v][2]), default=-1)
    val = {}
    if env and env.kind == "set":
        keys = env.C.K                                  # the set's own oracle and keys
    L = keys.L
    acc_words = m.level_words[2]

    def one(v):
        kind, p, ops, _ = m.nodes[v]
        a = [val[o] for o in ops]
        if kind == "const":
            return p
        if kind == "trgsw":
            w = m.records[p][2]
            return (env.trgsw(w) if isinstance(w, int) else w, None)
        if env and env.kind == "ring":                  # lvl0 gates on the N = 2048 ring
            if kind == "gate":
                arrs = [np.ascontiguousarray(x).reshape(1, -1) for x in a] + [None] * (3 - len(a))
                return env.keys2.gate_batch(np.array([ol.OPS.index(p[0])], np.int32), arrs[0], arrs[1], arrs[2], threads=1)[0]
            d = defs[p[0]] if kind in ("user", "multi") else None
            if kind == "user":
                return lc.user_gate_one(env.keys2, d[0], d[1], d[2], a)
            if kind == "multi":
                return [env.keys2.keyswitch(row) for row in mc2.multi_extract_one(env.keys2, d[0], d[1], d[2], d[3], a)]
        if env and env.kind == "set" and kind in ("refresh", "seiks_at"):
            # composed from the pieces load_set binds: SampleExtract(0), the key switch and, for Refresh, the rotation of the result
            t1 = np.zeros(m.level_words[1], np.uint32)
            L.orc_sample_extract0(t1, np.ascontiguousarray(a[0], np.uint32))
            t0 = keys.keyswitch(t1)
            return t0 if kind == "seiks_at" else keys.blind_rotate(t0)
        if env and env.kind == "set" and kind in ("user", "multi"):
            d = defs[p[0]]
            rows = env.C.user_gate_one(p[1], d[0], d[1], d[2], a, s=mc.shift_of(d[3]))
            return rows[0] if kind == "user" else list(rows)
        if kind == "gate":
            arrs = [np.ascontiguousarray(x).reshape(1, -1) for x in a] + [None] * (3 - len(a))
            return keys.gate_batch(ol.OPS.index(p[0]), p[1], arrs[0], arrs[1], arrs[2], threads=1)[0]
        if kind == "user":
            d = defs[p[0]]
            return uc.user_gate_one(keys, p[1], d[0], d[1], d[2], a)
        if kind == "multi":
            d = defs[p[0]]
            return mc.multi_gate_one(keys, p[1], d[0], d[1], d[2], d[3], a)
        if kind == "output":
            return a[0][p]
        if kind == "boot":
            return keys.blind_rotate(a[0])
        if kind == "refresh":
            r = np.zeros(acc_words, np.uint32)
            L.orc_refresh(keys.ek, r, np.ascontiguousarray(a[0]))
            return r
        if kind == "seiks_at":
            if p == 0:
                t0 = np.zeros(m.level_words[0], np.uint32)
                L.orc_sample_extract_keyswitch(keys.ek, t0, np.ascontiguousarray(a[0]))
                return t0
            return pr.extract_keyswitch(keys, a[0], p)
        if kind == "cmux" and env and env.kind == "set":
            res = np.zeros(acc_words, np.uint32)
            L.orc_cmux(res, np.ascontiguousarray(a[2][0], np.uint32), np.ascontiguousarray(a[0], np.uint32), np.ascontiguousarray(a[1], np.uint32))
            return res
        if kind == "cmux":
            return pr.cmux(L, a[2][0], a[0], a[1])
        if kind == "cmuxrot":
            return pr.cmux_rotate(L, a[1][0], a[0], p)
        raise ValueError(kind)

    with ThreadPoolExecutor(threads) as ex:
        for dd in range(max(depth.values(), default=-1) + 1):
            layer = [v for v in need if depth[v] == dd]
            cbs = [v for v in layer if m.nodes[v][0] == "cb"]
            if cbs:
                if cb_oracle is None:
                    raise RuntimeError("the program holds circuit bootstraps: evaluate needs cb_oracle")
                for v, tn in zip(cbs, cb_oracle([val[m.nodes[v][2][0]] for v in cbs])):
                    val[v] = tn
            rest = [v for v in layer if m.nodes[v][0] != "cb"]
            for v, w in zip(rest, ex.map(one, rest)):
                val[v] = w
    return val


def describe(m, v):
    """the record that made value v, and the records that made its operands"""
    kind, p, ops, r = m.nodes[v]

    def short(rec):
        return tuple(x if not isinstance(x, (np.ndarray, dict)) else "..." for x in rec)
    text = "value %d (%s) made by record #%d %s" % (v, kind, r, short(m.records[r]) if r >= 0 else "(initial host words)")
    for o in ops:
        ro = m.nodes[o][3]
        text += "\n    operand value %d (%s) made by record #%d %s" % (o, m.nodes[o][0], ro, short(m.records[ro]) if ro >= 0 else "(initial host words)")
    return text


# ---- issue on the device ----
def issue(api, m, ops, env=None):
    """plays m.records through cufhe_amd.api; `ops` are the op ids of user_defs() as api.define_gate returned them.  Returns
    (ctxts, observations, ntt): observations = [(label, name, observed words, expected vid)], ntt = {vid of a TRGSW2NTT value: the words the
    library wrote to the holder's host member}."""
    out_op = api.user_op_output if env is None else api.lvl2_user_op_output if env.kind == "ring" else api.ps_user_op_output
    cls = {0: lambda: api.Ctxt(0), 1: lambda: api.Ctxt(1), 2: api.Trlwe, 3: api.TrgswNtt}
    ct = {x: cls[x[0]]() for x in m.names}
    k = 0                                 # (the initial host words are the first nodes of the model, in the order of m.names)
    for x in m.names:
        if x[0] != 3:
            ct[x].tlwehost[:] = m.nodes[k][1]
            k += 1
    nst = 1 + max([r[-1] for r in m.records if r[0] not in ("flush", "sync", "edit", "poll", "wait")] + [r[1] for r in m.records if r[0] in ("poll", "wait")])
    sts = [api.Stream() for _ in range(nst)]
    for s in sts:
        s.Create()
    fn = {nm: (getattr(api, nm[0] + nm[1:].lower().replace("ny", "NY").replace("yn", "YN")),
               getattr(api, "g" + nm[0] + nm[1:].lower().replace("ny", "NY").replace("yn", "YN"))) for nm in TWO}
    obs, ntt = [], {}
    trgsw_vid = {p: v for v, (kind, p, _, _) in enumerate(m.nodes) if kind == "trgsw"}

    def observe(label, snap):
        for x, v in snap.items():
            obs.append((label, x, ct[x].tlwehost.copy(), v))

    for i, rec in enumerate(m.records):
        kind = rec[0]
        if kind == "gate":
            _, nm, copying, out, ins, st = rec
            c = [ct[x] for x in ins]
            if nm == "NOT":
                (api.Not if copying else api.gNot)(ct[out], c[0], sts[st])
            elif nm == "MUX":
                (api.Mux if copying else api.gMux)(ct[out], c[0], c[1], c[2], sts[st])
            else:
                fn[nm][0 if copying else 1](ct[out], c[0], c[1], sts[st])
        elif kind == "user":
            _, d, copying, out, ins, st = rec
            (api.Apply if copying else api.gApply)(ops[d], ct[out], *[ct[x] for x in ins], sts[st])
        elif kind == "sib":
            _, d, j, copying, out, ins, st = rec
            (api.Apply if copying else api.gApply)(out_op(ops[d], j), ct[out], *[ct[x] for x in ins], sts[st])
        elif kind == "multi":
            _, d, copying, outs, ins, st = rec
            (api.ApplyMulti if copying else api.gApplyMulti)(ops[d], [ct[o] for o in outs], *[ct[x] for x in ins], sts[st])
        elif kind == "boot":
            _, copying, out, x, st = rec
            (api.GateBootstrappingTLWE2TRLWElvl01NTT if copying else api.gGateBootstrappingTLWE2TRLWElvl01NTT)(ct[out], ct[x], sts[st])
        elif kind == "refresh":
            _, copying, out, x, st = rec
            (api.Refresh if copying else api.gRefresh)(ct[out], ct[x], sts[st])
        elif kind == "seiks_at":
            _, j, copying, out, x, st = rec
            if copying:
                api.SampleExtractAndKeySwitch(ct[out], ct[x], sts[st], index=j)
            elif j:
                api.gSampleExtractAndKeySwitch(ct[out], ct[x], sts[st], index=j)
            else:
                api._trlwe_op(api.TL_SEIKS, False, ct[out], ct[x], sts[st])
        elif kind == "cmux":
            _, copying, res, cs, c1, c0, st = rec
            (api.CMUXNTT if copying else api.gCMUXNTT)(ct[res], ct[cs], ct[c1], ct[c0], sts[st])
        elif kind == "cmuxrot":
            _, e, copying, res, cs, c, st = rec
            (api.CMUXRotateNTT if copying else api.gCMUXRotateNTT)(ct[res], ct[cs], ct[c], e, sts[st])
        elif kind == "cb":
            _, copying, out, x, st = rec
            (api.CircuitBootstrapping if copying else api.gCircuitBootstrapping)(ct[out], ct[x], sts[st])
        elif kind == "ntt":
            _, h, words, st = rec
            api.TRGSW2NTT(ct[h], env.trgsw(words) if isinstance(words, int) else words, sts[st])
            ntt[trgsw_vid[i]] = ct[h].tlwehost.copy()
        elif kind == "h2d":
            api.CtxtCopyH2D(ct[rec[1]], sts[rec[2]])
        elif kind == "d2h":
            api.CtxtCopyD2H(ct[rec[1]], sts[rec[2]])
        elif kind in ("poll", "wait"):
            done = api.StreamQuery(sts[rec[1]])
            polls = 1
            while kind == "wait" and not done and polls < 50000000:      # (as test/test_intensive.cc polls; bounded, so that a lost completion fails)
                done = api.StreamQuery(sts[rec[1]])
                polls += 1
            assert done or kind == "poll", "StreamQuery of stream %d never returned true (record #%d)" % (rec[1], i)
            if done:
                observe("after StreamQuery of stream %d at record #%d" % (rec[1], i), rec[2])
        elif kind == "flush":
            api.Flush(0)
        elif kind == "sync":
            api.Synchronize()
            observe("after Synchronize at record #%d" % i if i < len(m.records) - 1 else "at the end", rec[1])
        elif kind == "edit":
            ct[rec[1]].tlwehost[:] = rec[2]
    for s in sts:
        s.Destroy()
    return ct, obs, ntt


def compare(m, obs, ntt, val):
    """None, or the message of the first observation that differs from the model"""
    for label, x, got, v in obs:
        want = val[v]
        if isinstance(want, tuple):                     # a TRGSW value: the NTT-domain words
            want = want[1] if want[1] is not None else ntt[v]
        if not np.array_equal(got, want):
            bad = int(np.flatnonzero(got != want)[0])
            return "%s: ciphertext %s (level %d, #%d) differs from the in-order model at word %d (%d of %d words differ)\n  expected %s" % (
                label, x, x[0], x[1], bad, int(np.count_nonzero(got != want)), got.size, describe(m, v))
    return None
