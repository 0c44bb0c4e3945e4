"""Multi-output user gates against single-output ones on the GPU (profiles/r08_multi_output_gates.md).  One process, runs alternated:
  - a level-0 batch of 8192 outputs: 4096 evaluations of a 2-output gate (one gate_list, siblings fused: 4096 rotations, 8192 key
    switches) against the same 8192 outputs as single-output user gates (8192 rotations) -- ms per batch;
  - 256 16-bit ripple-carry adders through the per-gate API (copying gates, one stream per adder, Synchronize at the end): one 2-output
    gate per bit (ApplyMulti: sum and carry of x = a + b + cin on b / 8 encodings) against the MAJ / XOR3 user-gate form (2 per bit)
    -- ms per 256 adders, issue time included, and the rotations per adder counted by the device profile.
Prints markdown tables.  Keys and ciphertexts come from the CPU oracle (seeded); every adder sum is decrypted and checked."""
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cufhe_amd as eng  # noqa: E402
import multi_output_checker as mc  # noqa: E402
import oracle_lib as ol  # noqa: E402
import user_gate_checker as uc  # noqa: E402
from tools.user_gate_times import Adders, fmt  # noqa: E402

api = eng.api
MU = ol.MU


def batch_times(keys, reps):
    count, W = 4096, ol.LVL_WORDS[0]
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2, size=(3, count))
    ins = [api.DeviceBuffer(count * W).upload(uc.encrypt_torus(keys, 0, bits[i].astype(np.uint64) * MU, 2.0 ** 17, 10 + i))
           for i in range(3)]
    out = api.DeviceBuffer(2 * count * W)
    fa = eng.define_gate((1, 1, 1), 0, mc.full_adder_tv(2), nout=2)
    sum_vals = np.array([(m & 1) * MU for m in range(4)], np.uint32)
    carry_vals = np.array([(m >> 1) * MU for m in range(4)], np.uint32)
    s_op = eng.define_gate((1, 1, 1), 0, eng.test_vector(sum_vals))
    c_op = eng.define_gate((1, 1, 1), 0, eng.test_vector(carry_vals))
    ptr_in = [[b.ptr + (g % count) * W * 4 for g in range(2 * count)] for b in ins]
    outs = [out.ptr + g * W * 4 for g in range(2 * count)]
    forms = {"2-output gate (4096 rotations)": [fa] * count + [eng.user_op_output(fa, 1)] * count,
             "single-output gates (8192 rotations)": [s_op] * count + [c_op] * count}
    arr = lambda ps: (ctypes.c_void_p * (2 * count))(*ps)  # noqa: E731
    args = {k: (np.array(v, np.int32), arr(outs), arr(ptr_in[0]), arr(ptr_in[1]), arr(ptr_in[2])) for k, v in forms.items()}

    def run(k):
        ops, o, a, b, c = args[k]
        eng.check(eng.lib.cufhe_amd_gate_list(0, None, 0, 2 * count, ops.ctypes.data, o, a, b, c))
        eng.Synchronize()

    for k in forms:
        run(k)
    results = {}
    for k in forms:                       # both forms decrypt to sum and carry (their words differ: other rounding, other test vector)
        run(k)
        results[k] = mc.decode(keys, 0, out.download().reshape(2 * count, W))
    x = bits.sum(axis=0)
    same = all(np.array_equal(v, np.concatenate([x & 1, x >> 1])) for v in results.values())
    t = {k: [] for k in forms}
    for _ in range(reps):
        for k in forms:
            t0 = time.perf_counter()
            run(k)
            t[k].append((time.perf_counter() - t0) * 1e3)
    return t, same


class MultiAdders(Adders):
    """the same adders on b / 8 encodings, one ApplyMulti per bit"""

    def __init__(self, keys, A=256, B=16, seed=0):
        super().__init__(keys, A, B, seed)
        sig = 2.0 ** 17
        bits = lambda v: np.array([(int(v[i]) >> k) & 1 for i in range(A) for k in range(B)], np.uint64)  # noqa: E731
        for cts, words in ((self.x, uc.encrypt_torus(keys, 0, bits(self.va) * MU, sig, seed + 5)),
                           (self.y, uc.encrypt_torus(keys, 0, bits(self.vb) * MU, sig, seed + 6))):
            for c, row in zip(cts, words):
                c.tlwehost[:] = row
        zero = uc.encrypt_torus(keys, 0, np.zeros(A, np.uint64), sig, seed + 7)
        for i in range(A):
            self.c[i * (B + 1)].tlwehost[:] = zero[i]

    def run(self, fa):
        A, B, x, y, s, c = self.A, self.B, self.x, self.y, self.s, self.c
        api.Synchronize()
        t0 = time.perf_counter()
        for k in range(B):
            for i in range(A):
                api.ApplyMulti(fa, [s[i * B + k], c[i * (B + 1) + k + 1]], x[i * B + k], y[i * B + k], c[i * (B + 1) + k], self.sts[i])
        t_issue = time.perf_counter()
        api.Synchronize()
        t1 = time.perf_counter()
        dec = lambda o: int(mc.decode(self.keys, 0, o.tlwehost)[0])  # noqa: E731
        got = [sum(dec(s[i * B + k]) << k for k in range(B)) + (dec(c[i * (B + 1) + B]) << B) for i in range(A)]
        ok = got == [int(self.va[i] + self.vb[i]) for i in range(A)]
        return (t1 - t0) * 1e3, (t_issue - t0) * 1e3, B, ok


def rotations(fn):
    api.profile_enable(True)
    api.profile_get(reset=True)
    r = fn()
    p = api.profile_get(reset=True)
    api.profile_enable(False)
    return r, p.blind_rotations


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    keys = ol.Keys(ol.load(), seed=1)
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    print(f"device: {api.device_identity()}  cus: {api.device_cus()}\n")
    bt, same = batch_times(keys, reps)
    print("## 8192 outputs at level 0 in one gate_list (ms per batch: median (min - max) over", reps, "alternated repetitions)\n")
    print("| form | ms |\n|---|---|")
    for k, v in bt.items():
        print(f"| {k} | {fmt(v)} |")
    print(f"\nboth forms decrypt to sum and carry: {same}")
    maj, xor3 = eng.define_gate((1, 1, 1), 0), eng.define_gate((2, 2, 2), 4 * ol.MU)
    fa = eng.define_gate((1, 1, 1), 0, mc.full_adder_tv(2), nout=2)
    res = {"MAJ/XOR3": [], "2-output gate": []}
    issue = {k: [] for k in res}
    rots, oks = {}, []
    add = Adders(keys, seed=100)
    madd = MultiAdders(keys, seed=200)
    for r in range(3):
        for name in res:
            if name == "MAJ/XOR3":
                (ms, ims, _, ok), nrot = rotations(lambda: add.run((maj, xor3)))
            else:
                (ms, ims, _, ok), nrot = rotations(lambda: madd.run(fa))
            res[name].append(ms)
            issue[name].append(ims)
            rots[name] = nrot / (add.A if name == "MAJ/XOR3" else madd.A)
            oks.append(ok)
    print("\n## 256 16-bit ripple-carry adders, per-gate API (copying gates; ms from the first enqueue to Synchronize, median (min - max)"
          " over 3 alternated runs)\n")
    print("| form | rotations per adder | ms per 256 adders | of which issuing (Python) |\n|---|---|---|---|")
    for k in res:
        print(f"| {k} | {rots[k]:g} | {fmt(res[k])} | {fmt(issue[k])} |")
    print(f"\nall sums decrypted right: {all(oks)}")
    eng.CleanUp()
    return 0 if all(oks) and same else 1


if __name__ == "__main__":
    sys.exit(main())
