"""The reference of the RECORDED pack (cufhe_amd_enqueue_pack) in numpy: pack_checker composed over a value
DAG.  A program is a list of ops over numbered slots -- lvl0 ciphertexts "c" and TRLWEs "t" -- evaluated in ISSUE order: every op reads
the values its operands hold when it is issued, which is what the scheduler owes its caller however it batches the ops into levels.

    pack      tout, ins [c slots, in term order; a slot may repeat], pos [0 <= pos < N, may repeat]
              t[tout] = sum_m X^pos[m] PackKS(c[ins[m]])          pack_checker.pack_ks / rotate, mod 2^32
    nand      out, a, b                                            the oracle's gate (keys.gate_batch)
    spread    tout, tin, stride, reps                              lut_checker.spread
    lookup    out, table, a                                        lut_checker.lut_lookup, one output, the address is c[a]

PackKS of one input is the costly part (up to n t rows of the key): it is computed once per distinct input words and shared."""
import numpy as np

import oracle_lib as ol
import pack_checker as pk

N, n = ol.N, ol.n
M32 = np.uint64(0xFFFFFFFF)
NAND = 0


class Model:
    def __init__(self, key, keys=None, rows=n):
        self.key, self.keys, self.rows = key, keys, rows
        self._ks = {}

    def pack_ks(self, x):
        x = np.ascontiguousarray(x, np.uint32)
        k = x.tobytes()
        if k not in self._ks:
            self._ks[k] = pk.pack_ks(self.key, x, self.rows)
        return self._ks[k]

    def pack(self, ins, pos):
        """sum_m X^pos[m] PackKS(ins[m]): [2N] uint32"""
        assert 1 <= len(ins) == len(pos) <= N
        out = np.zeros(2 * N, np.uint64)
        for x, p in zip(ins, pos):
            assert 0 <= int(p) < N
            out += pk.rotate(self.pack_ks(x), int(p))
        return (out & M32).astype(np.uint32)

    def run(self, c, t, prog):
        """c, t: lists of initial slot words (copied).  Returns (c, t) after the program."""
        c, t = [np.array(x, np.uint32) for x in c], [np.array(x, np.uint32) for x in t]
        for op in prog:
            kind = op["kind"]
            if kind == "pack":
                t[op["tout"]] = self.pack([c[i] for i in op["ins"]], op["pos"])
            elif kind == "nand":
                c[op["out"]] = self.keys.gate_batch(NAND, 0, c[op["a"]][None, :], c[op["b"]][None, :])[0]
            elif kind == "spread":
                import lut_checker as lc
                t[op["tout"]] = lc.spread(t[op["tin"]], op["stride"], op["reps"])
            elif kind == "lookup":
                import lut_checker as lc
                c[op["out"]] = lc.lut_lookup(self.keys, c[op["a"]], t[op["table"]], 1)[0]
            else:
                raise ValueError(kind)
        return c, t
