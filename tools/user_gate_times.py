"""User gates against built-in ones on the GPU (profiles/r07_user_gates.md).  One process, runs alternated:
  - a 4096-gate batch at level 0: NAND, a user gate with NAND's numbers and no test vector, the same with a table test vector
    (cufhe_amd_test_vector, p = 4) -- ms per batch over the repetitions;
  - 256 16-bit ripple-carry adders through the per-gate API (copying gates, one stream per adder, Synchronize at the end): the
    5-gate form (Xor, Xor, And, And, Or per bit) against the MAJ / XOR3 user-gate form (2 per bit) -- ms per 256 adders, issue
    time included (Python enqueue calls), and the bootstraps per adder.
Prints markdown tables (profiles/r07_user_gates.md).  Keys and ciphertexts come from the CPU oracle (seeded); every adder sum is
decrypted and checked."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cufhe_amd as eng  # noqa: E402
import oracle_lib as ol  # noqa: E402

api = eng.api


def batch_times(keys, reps):
    count, W = 4096, ol.LVL_WORDS[0]
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2, size=(2, count)).astype(np.uint8)
    a = api.DeviceBuffer(count * W).upload(keys.encrypt(bits[0], 0, seed=1))
    b = api.DeviceBuffer(count * W).upload(keys.encrypt(bits[1], 0, seed=2))
    out = api.DeviceBuffer(count * W)
    mu = ol.MU
    tv = eng.test_vector(np.array([1, 3, 0, 2], np.uint64) * mu)
    ops = {"NAND (built-in)": api.NAND,
           "user gate, NAND numbers, no TV": eng.define_gate((-1, -1, 0), mu),
           "user gate, NAND numbers, table TV": eng.define_gate((-1, -1, 0), mu, tv)}
    t = {k: [] for k in ops}
    for name, op in ops.items():          # warm-up
        eng.gate_batch(op, 0, out, a, b, count=count)
    eng.Synchronize()
    for _ in range(reps):
        for name, op in ops.items():
            t0 = time.perf_counter()
            eng.gate_batch(op, 0, out, a, b, count=count)
            eng.Synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3)
    return t


class Adders:
    """A B-bit ripple-carry adders on host-resident ciphertexts, one stream each: created once, run in either form"""

    def __init__(self, keys, A=256, B=16, seed=0):
        rng = np.random.default_rng(seed)
        self.keys, self.A, self.B = keys, A, B
        self.va, self.vb = rng.integers(0, 1 << B, A), rng.integers(0, 1 << B, A)
        ex = keys.encrypt(np.array([(self.va[i] >> k) & 1 for i in range(A) for k in range(B)], np.uint8), 0, seed=seed + 1)
        ey = keys.encrypt(np.array([(self.vb[i] >> k) & 1 for i in range(A) for k in range(B)], np.uint8), 0, seed=seed + 2)
        zero = keys.encrypt(np.zeros(A, np.uint8), 0, seed=seed + 3)
        self.x, self.y = [api.Ctxt(0) for _ in range(A * B)], [api.Ctxt(0) for _ in range(A * B)]
        for c, row in zip(self.x, ex):
            c.tlwehost[:] = row
        for c, row in zip(self.y, ey):
            c.tlwehost[:] = row
        self.s = [api.Ctxt(0) for _ in range(A * B)]
        self.c = [api.Ctxt(0) for _ in range(A * (B + 1))]      # c[i (B + 1) + k]: carry into bit k of adder i (inputs are never written)
        for i in range(A):
            self.c[i * (B + 1)].tlwehost[:] = zero[i]
        self.t1, self.t2 = [api.Ctxt(0) for _ in range(A)], [api.Ctxt(0) for _ in range(A)]
        self.sts = [api.Stream() for _ in range(A)]
        for st in self.sts:
            st.Create()

    def run(self, form):
        """ms from the first enqueue to Synchronize, of which issuing; bootstraps per adder; sums right"""
        A, B, x, y, s, c = self.A, self.B, self.x, self.y, self.s, self.c
        api.Synchronize()
        t0 = time.perf_counter()
        for k in range(B):
            for i in range(A):
                X, Y, S, C, Cn, st = x[i * B + k], y[i * B + k], s[i * B + k], c[i * (B + 1) + k], c[i * (B + 1) + k + 1], self.sts[i]
                if form == "5-gate":
                    api.Xor(self.t1[i], X, Y, st)
                    api.Xor(S, self.t1[i], C, st)
                    api.And(self.t2[i], self.t1[i], C, st)
                    api.And(self.t1[i], X, Y, st)
                    api.Or(Cn, self.t1[i], self.t2[i], st)
                else:
                    api.Apply(form[1], S, X, Y, C, st)
                    api.Apply(form[0], Cn, X, Y, C, st)
        t_issue = time.perf_counter()
        api.Synchronize()
        t1 = time.perf_counter()
        dec = lambda o: int(self.keys.decrypt(o.tlwehost, 0)[0])  # noqa: E731
        got = [sum(dec(s[i * B + k]) << k for k in range(B)) + (dec(c[i * (B + 1) + B]) << B) for i in range(A)]
        ok = got == [int(self.va[i] + self.vb[i]) for i in range(A)]
        return (t1 - t0) * 1e3, (t_issue - t0) * 1e3, (5 if form == "5-gate" else 2) * B, ok


def fmt(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} - {max(v):.2f})"


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    keys = ol.Keys(ol.load(), seed=1)
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    print(f"device: {api.device_identity()}  cus: {api.device_cus()}\n")
    bt = batch_times(keys, reps)
    print("## 4096-gate batch, level 0 (ms per batch: median (min - max) over", reps, "alternated repetitions)\n")
    print("| gate | ms |\n|---|---|")
    for k, v in bt.items():
        print(f"| {k} | {fmt(v)} |")
    maj, xor3 = eng.define_gate((1, 1, 1), 0), eng.define_gate((2, 2, 2), 4 * ol.MU)
    res = {"5-gate": [], "MAJ/XOR3": []}
    issue = {"5-gate": [], "MAJ/XOR3": []}
    boots, oks = {}, []
    add = Adders(keys, seed=100)
    for r in range(3):
        for name, form in (("5-gate", "5-gate"), ("MAJ/XOR3", (maj, xor3))):
            ms, ims, bpa, ok = add.run(form)
            res[name].append(ms)
            issue[name].append(ims)
            boots[name] = bpa
            oks.append(ok)
    print("\n## 256 16-bit ripple-carry adders, per-gate API (copying gates; ms from the first enqueue to Synchronize, median (min - max)"
          " over 3 alternated runs)\n")
    print("| form | bootstraps per adder | ms per 256 adders | of which issuing (Python) |\n|---|---|---|---|")
    for k in res:
        print(f"| {k} | {boots[k]} | {fmt(res[k])} | {fmt(issue[k])} |")
    print(f"\nall sums decrypted right: {all(oks)}")
    eng.CleanUp()
    return 0 if all(oks) else 1


if __name__ == "__main__":
    sys.exit(main())
