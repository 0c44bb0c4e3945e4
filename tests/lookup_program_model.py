"""The reference of the RECORDED lookups, Spreads and table rotations (cufhe_amd_enqueue_lookup / _enqueue_spread /
_enqueue_lut_rotate), in numpy over the existing checkers, and a generator of small random dependent
programs over them and the ops they meet in a netlist.

A lookup definition is (c0, c1, offset, nout).  Its address is
    x = (c0 in0 + c1 in1 + (0, ..., 0, offset)) mod 2^32
and its outputs are lut_checker.lut_lookup(keys, x, table, nout); Spread is lut_checker.spread, the rotation lut_checker.lut_rotate.
With (1, 0), offset 0 the address IS in0, so the model is lut_checker.lut_lookup on the same words by construction.

Programs are lists of ops over numbered slots -- lvl0 ciphertexts "c" and TRLWEs "t" -- evaluated in ISSUE order as a value DAG:
every op reads the values its operands hold when it is issued.  That is the semantics the scheduler owes its caller, however it
batches the ops into levels."""
import numpy as np

import lut_checker as lc
import multi_output_checker as mc
import oracle_lib as ol
import packed_rom_checker as pr
import user_gate_checker as uc

N, n = ol.N, ol.n
M32 = np.uint64(0xFFFFFFFF)


def address(c0, c1, offset, in0, in1=None):
    """x = c0 in0 + c1 in1 + (0, .., 0, offset) mod 2^32 on lvl0 ciphertexts (n + 1 words)"""
    x = np.asarray(in0, np.uint32).astype(np.uint64) * np.uint64(c0 & 0xFFFFFFFF)
    if c1 != 0:
        x = x + np.asarray(in1, np.uint32).astype(np.uint64) * np.uint64(c1 & 0xFFFFFFFF)
    x[n] += np.uint64(offset & 0xFFFFFFFF)
    return (x & M32).astype(np.uint32)


def lookup(keys, defn, table, in0, in1=None):
    """[nout][n + 1]: every output of Lookup(defn, table, in0, in1), defn = (c0, c1, offset, nout)"""
    c0, c1, offset, nout = defn
    return lc.lut_lookup(keys, address(c0, c1, offset, in0, in1), table, nout)


def lut_rotate(keys, table, addr, nout=1):
    return lc.lut_rotate(keys, addr, table, mc.shift_of(nout))


spread = lc.spread

def worked_example_inputs(keys, seed=2500):
    """the committed case: entries v, the TRLWE holding (2 v[m] - 1) / 8 at coefficient m N / 4 (sigma 2^-25), the padded addresses
    m / 8 (sigma 2^-15).  tests/test_recorded_lut.py checks on the checker alone that every address reads its entry."""
    v = np.random.default_rng(seed).integers(0, 2, size=4).astype(np.uint8)
    v[0], v[3] = 1, 0                                   # both values occur
    msgs = np.zeros(N, np.uint32)
    msgs[np.arange(4) * (N // 4)] = np.where(v == 1, ol.MU, (1 << 32) - ol.MU).astype(np.uint32)
    table_words = pr.encrypt_trlwe(keys, msgs, 2.0 ** 7, seed + 1)
    addrs = uc.encrypt_torus(keys, 0, np.arange(4, dtype=np.uint64) * np.uint64(ol.MU), 2.0 ** 17, seed + 2)
    return table_words, addrs, v


# ---- random dependent programs ----
# ops (dicts): kind and
#   nand      out, a, b            lvl0 slots
#   user      out, a               the program's one user gate (coefficients (1, 0, 0), USER_OFFSET, USER_TV), one operand
#   copy      out, a
#   lookup    d (index into DEFS), outs [(slot, j), ...] in REQUEST order, table (t slot), a, b (None for one-operand definitions)
#   spread    tout, tin, stride, reps
#   lutrot    tout, tin, a, nout
#   seiks_at  out, tin, j          SampleExtractAndKeySwitch at coefficient j
DEFS = [(1, 0, 0, 1), (1, 1, 0x13572468, 1), (1, 0, 0, 2), (-1, 1, 0x9ABCDEF0, 8), (1, 0, 0, 8)]
SPREADS = [(1, 256), (2, 128), (8, 16), (1, 1), (1024, 1), (1, 1024)]
USER_OFFSET = ol.MU
HAZARDS = ("address_from_gate", "table_from_spread", "spread_over_read_table", "in_place_lookup", "siblings_out_of_order",
           "one_definition_two_tables")
NC, NT = 14, 4


def user_tv():
    return np.random.default_rng(2300).integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)


def generate(seed, ops=40):
    """one program: the initial words of its slots and its op list.  Each hazard class is planted once at a random place; the rest
    is drawn at random, outputs and operands from all slots, so further hazards of every kind arise by themselves."""
    rng = np.random.default_rng(seed)
    init_c = rng.integers(0, 1 << 32, size=(NC, n + 1), dtype=np.uint64).astype(np.uint32)
    init_t = rng.integers(0, 1 << 32, size=(NT, 2 * N), dtype=np.uint64).astype(np.uint32)
    prog = []

    def c():
        return int(rng.integers(NC))

    def t():
        return int(rng.integers(NT))

    def other_t(x):
        return int((x + 1 + rng.integers(NT - 1)) % NT)

    def a_lookup(d=None, table=None, a=None, outs=None):
        d = int(rng.integers(len(DEFS))) if d is None else d
        c0, c1, off, nout = DEFS[d]
        a = c() if a is None else a
        b = c() if c1 != 0 else None
        if outs is None:
            if nout == 1:
                outs = [(c(), 0)]
            else:       # nout distinct slots, none of them an operand
                free = [s for s in rng.permutation(NC) if s not in (a, b)]
                outs = [(int(free[j]), j) for j in range(nout)]
        return {"kind": "lookup", "d": d, "outs": outs, "table": t() if table is None else table, "a": a, "b": b}

    def random_op():
        k = rng.choice(["nand", "user", "copy", "lookup", "lookup", "spread", "lutrot", "seiks_at"])
        if k == "nand":
            return {"kind": "nand", "out": c(), "a": c(), "b": c()}
        if k in ("user", "copy"):
            return {"kind": str(k), "out": c(), "a": c()}
        if k == "lookup":
            return a_lookup()
        if k == "spread":
            tin = t()
            stride, reps = SPREADS[int(rng.integers(len(SPREADS)))]
            return {"kind": "spread", "tout": other_t(tin), "tin": tin, "stride": stride, "reps": reps}
        if k == "lutrot":
            tin = t()
            return {"kind": "lutrot", "tout": other_t(tin), "tin": tin, "a": c(), "nout": int(rng.choice([1, 2, 8]))}
        return {"kind": "seiks_at", "out": c(), "tin": t(), "j": int(rng.integers(N))}

    # the planted hazards, each a short run of ops
    g, tt = c(), t()
    plant = [
        [{"kind": "nand", "out": g, "a": c(), "b": c()}, a_lookup(d=0, a=g)],                                  # address from a gate
        [{"kind": "spread", "tout": tt, "tin": other_t(tt), "stride": 1, "reps": 256}, a_lookup(table=tt)],     # table from a Spread
        [a_lookup(d=2, table=tt), {"kind": "spread", "tout": tt, "tin": other_t(tt), "stride": 2, "reps": 128}],  # Spread over a read table
        [a_lookup(d=0, a=g, outs=[(g, 0)])],                                                                     # in place
    ]
    sib = a_lookup(d=4)
    sib["outs"] = [sib["outs"][j] for j in (5, 0, 3)]                                                         # siblings, j not rising
    plant.append([sib])
    a = c()
    first = a_lookup(d=2, table=tt, a=a)
    free = [int(s) for s in rng.permutation(NC) if s != a and s not in [o for o, _ in first["outs"]]]
    plant.append([first, a_lookup(d=2, table=other_t(tt), a=a, outs=[(free[0], 0), (free[1], 1)])])          # one definition, two tables
    fill = max(0, ops - sum(len(p) for p in plant))
    cuts = sorted(rng.integers(0, fill + 1, size=len(plant)))
    order = rng.permutation(len(plant))
    done = 0
    for i, cut in enumerate(cuts):
        while done < cut:
            prog.append(random_op())
            done += 1
        prog.extend(plant[order[i]])
    while done < fill:
        prog.append(random_op())
        done += 1
    return init_c, init_t, prog


def hazards(prog):
    """how often each hazard class occurs in a program, found from the op list alone"""
    count = dict.fromkeys(HAZARDS, 0)
    c_writer = {}           # lvl0 slot -> kind of the op that last wrote it
    t_writer = {}           # TRLWE slot -> kind of the op that last wrote it
    t_lookup_reads = set()  # TRLWE slots a lookup has read since their last write
    prev = None
    for op in prog:
        k = op["kind"]
        if k == "lookup":
            if c_writer.get(op["a"]) in ("nand", "user") or (op["b"] is not None and c_writer.get(op["b"]) in ("nand", "user")):
                count["address_from_gate"] += 1
            if t_writer.get(op["table"]) == "spread":
                count["table_from_spread"] += 1
            nout = DEFS[op["d"]][3]
            if nout == 1 and op["outs"][0][0] == op["a"]:
                count["in_place_lookup"] += 1
            js = [j for _, j in op["outs"]]
            if any(js[i + 1] <= js[i] for i in range(len(js) - 1)):
                count["siblings_out_of_order"] += 1
            if prev is not None and prev["kind"] == "lookup" and prev["d"] == op["d"] and prev["table"] != op["table"] and \
                    not {s for s, _ in prev["outs"]} & {op["a"], op["b"]} and not {s for s, _ in prev["outs"]} & {s for s, _ in op["outs"]}:
                count["one_definition_two_tables"] += 1       # independent neighbours: they share a dependence level
            t_lookup_reads.add(op["table"])
            for s, _ in op["outs"]:
                c_writer[s] = k
        elif k in ("spread", "lutrot"):
            if k == "spread" and op["tout"] in t_lookup_reads:
                count["spread_over_read_table"] += 1
            t_lookup_reads.discard(op["tout"])
            t_writer[op["tout"]] = k
        else:
            c_writer[op["out"]] = k
        prev = op
    return count


def evaluate(keys, init_c, init_t, prog):
    """final words of every slot, ops applied in issue order"""
    cv, tv = init_c.copy(), init_t.copy()
    utv = user_tv()
    for op in prog:
        k = op["kind"]
        if k == "nand":
            cv[op["out"]] = keys.gate_batch(ol.OPS.index("NAND"), 0, cv[op["a"]][None], cv[op["b"]][None])[0]
        elif k == "user":
            cv[op["out"]] = uc.user_gate_one(keys, 0, (1, 0, 0), USER_OFFSET, utv, [cv[op["a"]]])
        elif k == "copy":
            cv[op["out"]] = cv[op["a"]]
        elif k == "lookup":
            res = lookup(keys, DEFS[op["d"]], tv[op["table"]], cv[op["a"]], None if op["b"] is None else cv[op["b"]])
            for s, j in op["outs"]:
                cv[s] = res[j]
        elif k == "spread":
            tv[op["tout"]] = spread(tv[op["tin"]], op["stride"], op["reps"])
        elif k == "lutrot":
            tv[op["tout"]] = lut_rotate(keys, tv[op["tin"]], cv[op["a"]], op["nout"])
        elif k == "seiks_at":
            cv[op["out"]] = pr.extract_keyswitch(keys, tv[op["tin"]], op["j"])
        else:
            raise ValueError(k)
    return cv, tv
