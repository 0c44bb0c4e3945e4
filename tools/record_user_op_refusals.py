#!/usr/bin/env python3
"""The refusal matrix of the user-gate op ids: which id is admitted where, and what a refusal says.

Every case sends one op id (or an ordered pair of bad ids of two families) through one entry point of the library while the gates take
one route, and records the call's return code and cufhe_amd_last_error().  Only the public C ABI and cufhe_amd.api are used, so the
same file runs on any commit:

    python tools/record_user_op_refusals.py            # writes tests/golden/user_op_refusals_v1.json (needs a GPU)

tests/test_gpu_user_op_refusals.py replays the matrix on the built library, tests/test_op_registry.py replays every row that needs no
launch on the CPU against cufhe_amd/csrc/op_registry.h.

The cases are the product  ids x routes x entries  plus  pairs x routes x list entries:
  ids      for each family (default, lvl2, ps): an undefined k, a defined single-output id, an output j >= nout of a multi-output
           definition, a valid output j > 0; for ps also an id defined for another set; for each of the four ranges (the lookups'
           included) the id below the base and the id at the range end
  routes   (param_set, lvl0_ring, level): the default path, the N = 2048 ring and an active set, each at level 0 and 1, and the set
           together with the ring at level 0
  entries  cufhe_amd_gate_list, the ring's batch, the set's batch, cufhe_amd_enqueue_gate with and without a second operand,
           cufhe_amd_enqueue_gate_multi, and the two parity hooks
  pairs    every ordered pair of bad ids (undefined k, output j >= nout, ps: another set's) of two different families, through the
           gate list and the two direct batch entries
An accepted case runs with count 1 on zero ciphertexts."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "user_op_refusals_v1.json")

USER_BASE, LVL2_BASE, PS_BASE, LOOKUP_BASE, CAP, OUTPUTS = 1000, 8192, 12288, 16384, 64, 8
FAMILY_BASE = {"default": USER_BASE, "lvl2": LVL2_BASE, "ps": PS_BASE}
SET, OTHER_SET = "k2n512", "default"          # the active set (the smallest compiled one) and the one "another set" means
UNDEFINED_K = 5

# definitions every family makes, in this order: row 0 a single-output gate of two operands, row 1 a two-output gate of two operands;
# the sets' table also has row 2, made for OTHER_SET.  name -> (family, row k, output j)
IDS = {}
for fam in ("default", "lvl2", "ps"):
    IDS[f"{fam}.undefined"] = (fam, UNDEFINED_K, 0)
    IDS[f"{fam}.single"] = (fam, 0, 0)
    IDS[f"{fam}.output_past_nout"] = (fam, 1, 2)
    IDS[f"{fam}.output1"] = (fam, 1, 1)
IDS["ps.other_set"] = ("ps", 2, 0)
EDGES = {}
for name, base in (("default", USER_BASE), ("lvl2", LVL2_BASE), ("ps", PS_BASE), ("lookup", LOOKUP_BASE)):
    EDGES[f"{name}.below_base"] = base - 1
    EDGES[f"{name}.range_end"] = base + CAP * OUTPUTS
BAD = [n for n in IDS if n.split(".")[1] in ("undefined", "output_past_nout", "other_set")]

# (name, param_set active, lvl0_ring, level)
ROUTES = [("default.l0", False, 1024, 0), ("default.l1", False, 1024, 1), ("ring.l0", False, 2048, 0), ("ring.l1", False, 2048, 1),
          ("set.l0", True, 1024, 0), ("set.l1", True, 1024, 1), ("set+ring.l0", True, 2048, 0)]
ENTRIES = ["gate_list", "ring_batch", "set_batch", "enqueue_gate.in1_null", "enqueue_gate", "enqueue_gate_multi", "lvl2_hook", "ps_hook"]
PAIR_ENTRIES = ["gate_list", "ring_batch", "set_batch"]


def op_id(name):
    if name in EDGES:
        return EDGES[name]
    fam, k, j = IDS[name]
    return FAMILY_BASE[fam] + k + j * CAP


def cases():
    """[(case name, entry, route, [id names])] in a fixed order"""
    out = []
    for route in ROUTES:
        for entry in ENTRIES:
            for name in list(IDS) + list(EDGES):
                out.append((f"{entry}|{route[0]}|{name}", entry, route, [name]))
        for entry in PAIR_ENTRIES:
            for a, b in itertools.permutations(BAD, 2):
                if a.split(".")[0] != b.split(".")[0]:
                    out.append((f"{entry}|{route[0]}|{a},{b}", entry, route, [a, b]))
    return out


EXPECTED_ROWS = len(ROUTES) * (len(ENTRIES) * (len(IDS) + len(EDGES)) + len(PAIR_ENTRIES) * 2 * (2 * 2 + 2 * 3 + 2 * 3))


class Matrix:
    """the engine with the session keys, the ring's keys, the two sets' keys and the definitions above; run(case) -> (rc, message)"""

    def __init__(self, eng, keys, keys2, set_keys):
        import numpy as np
        self.np, self.eng, self.api, self.lib = np, eng, eng.api, eng.lib
        api = self.api
        eng.CleanUp()
        eng.SetGPUNum(1)
        eng.Initialize(keys.bk, keys.ksk)
        api.lvl2_initialize(keys2.bk, keys2.ksk)
        self.set, other = api.ps_index(SET), api.ps_index(OTHER_SET)
        api.ps_initialize(self.set, set_keys.bk, set_keys.ksk)
        api.ps_initialize(other, keys.bk, keys.ksk)
        mu = 1 << 29
        two = [[mu, (0 - mu) & 0xFFFFFFFF], [0, 1 << 31]]
        assert api.define_gate((-1, -1, 0), mu) == USER_BASE
        assert api.define_gate((1, 1, 0), 0, api.test_vector_multi(two), nout=2) == USER_BASE + 1
        assert api.lvl2_define_gate((-1, -1, 0), mu) == LVL2_BASE
        two64 = (np.array(two, np.uint64) << np.uint64(32))
        assert api.lvl2_define_gate((1, 1, 0), 0, api.lvl2_test_vector_multi(two64), nout=2) == LVL2_BASE + 1
        assert api.ps_define_gate(self.set, (-1, -1, 0), mu) == PS_BASE
        assert api.ps_define_gate(self.set, (1, 1, 0), 0, api.ps_test_vector_multi(self.set, two), nout=2) == PS_BASE + 1
        assert api.ps_define_gate(other, (-1, -1, 0), mu) == PS_BASE + 2
        # operands: zero ciphertexts, room for two of any level of any route; the hooks' accumulators
        self.buf = [api.DeviceBuffer(4096).upload(np.zeros(4096, np.uint32)) for _ in range(4)]
        self.acc = api.DeviceBuffer(16384).upload(np.zeros(16384, np.uint32))
        self.route = None
        self.ctxts = []

    def close(self):
        self.use_route(("default.l0", False, 1024, 0))
        for c in self.ctxts:
            c.release()
        for b in self.buf + [self.acc]:
            b.free()
        self.eng.CleanUp()

    def use_route(self, route):
        if route == self.route:
            return
        api = self.api
        self.eng.Synchronize()
        for c in self.ctxts:
            c.release()
        api.set_option("param_set", self.set if route[1] else -1)
        api.set_option("lvl0_ring", route[2])
        # ciphertext handles of the route's level and of the active set's size: two outputs, three operands
        self.ctxts = [api.Ctxt(route[3]) for _ in range(5)]
        self.route = route

    def run(self, case):
        _, entry, route, names = case
        np, lib, api = self.np, self.lib, self.api
        self.use_route(route)
        level = route[3]
        ops = np.array([op_id(n) for n in names], np.int32)
        count = len(names)
        out, in0, in1, in2 = (ctypes.c_void_p(b.ptr) for b in self.buf)
        i32p = ops.ctypes.data
        if entry == "gate_list":
            words = lib.cufhe_amd_ctxt_words(level)
            arr = [(ctypes.c_void_p * count)(*[b.ptr + 4 * words * g for g in range(count)]) for b in self.buf]
            rc = lib.cufhe_amd_gate_list(0, None, level, count, i32p, *arr)
        elif entry == "ring_batch":
            rc = lib.cufhe_amd_lvl2_gate_batch(0, None, count, i32p, 1, out, in0, in1, in2, api.LVL_WORDS[0])
        elif entry == "set_batch":
            p = api.ps_params(self.set)
            rc = lib.cufhe_amd_ps_gate_batch_level(self.set, 0, None, level, count, i32p, 1, out, in0, in1, in2,
                                                   p.lvl1_words if level else p.lvl0_words)
        elif entry in ("enqueue_gate", "enqueue_gate.in1_null"):
            o0, _, a, b, c = (x._h for x in self.ctxts)
            if entry.endswith("in1_null"):
                b = c = None
            rc = lib.cufhe_amd_enqueue_gate(0, None, int(ops[0]), 0, o0, a, b, c)
        elif entry == "enqueue_gate_multi":
            o0, o1, a, b, c = (x._h for x in self.ctxts)
            rc = lib.cufhe_amd_enqueue_gate_multi(0, None, int(ops[0]), 0, 2, (ctypes.c_void_p * 2)(o0, o1), a, b, c)
        elif entry == "lvl2_hook":
            rc = lib.cufhe_amd_lvl2_user_rotate_batch(0, None, 1, int(ops[0]), in0, in1, in2, 1, ctypes.c_void_p(self.acc.ptr))
        elif entry == "ps_hook":
            rc = lib.cufhe_amd_ps_user_rotate(self.set, 0, None, 1, int(ops[0]), in0, in1, in2, ctypes.c_void_p(self.acc.ptr), 1)
        else:
            raise KeyError(entry)
        if rc == 0:          # accepted: the work it started must end well too
            rc = lib.cufhe_amd_synchronize()
        return int(rc), (lib.cufhe_amd_last_error().decode() if rc else "")


def session_keys():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as ol
    L = ol.load()
    keys = ol.Keys(L, seed=1)
    return keys, ol.KeysLvl2(L, keys, seed=7), ol.Keys(ol.load_set(SET), seed=5)


def record(path=FIXTURE):
    sys.path.insert(0, ROOT)
    import cufhe_amd as eng
    m = Matrix(eng, *session_keys())
    messages, rows = [""], []
    for case in cases():
        rc, msg = m.run(case)
        if msg not in messages:
            messages.append(msg)
        rows.append([case[0], rc, messages.index(msg)])
    m.close()
    assert len(rows) == EXPECTED_ROWS
    # RECORD_COMMIT: where the library was built from a tree without its history
    commit = os.environ.get("RECORD_COMMIT") or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                                               text=True).stdout.strip()
    what = ("return code and cufhe_amd_last_error() of every case of tools/record_user_op_refusals.py, recorded on an MI355X from the "
            f"library of commit {commit}; a row is [case, code, index into messages]; see profiles/r26_op_registry.md")
    with open(path, "w") as f:
        f.write('{\n "what": %s,\n "messages": [\n  %s\n ],\n "rows": [\n  %s\n ]\n}\n' % (
            json.dumps(what), ",\n  ".join(json.dumps(m) for m in messages), ",\n  ".join(json.dumps(r) for r in rows)))
    print(f"{len(rows)} rows, {len(messages) - 1} distinct messages, {sum(1 for r in rows if r[1] == 0)} accepted -> {path}")


if __name__ == "__main__":
    record(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
