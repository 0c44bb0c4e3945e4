"""User gates of the N = 2048 ring against the ring's built-in gates on the GPU (profiles/r14_lvl2_user_gates.md).  One process, runs
alternated: a 4096-gate batch through cufhe_amd_lvl2_gate_batch of
  - NAND (built-in: the <false> instantiation of the rotation kernel),
  - a lvl2 user gate with NAND's numbers and no test vector (pad 0, still <false>),
  - the same with a table test vector (cufhe_amd_lvl2_test_vector, p = 8: the <true> instantiation, 8 gathered words per lane before
    the 630 steps),
  - the table gate without its key switch (cufhe_amd_lvl2_user_extract_batch)
-- ms per batch over the repetitions.  Prints a markdown table.  Keys and ciphertexts come from the CPU oracle (seeded); the table
gate's outputs are decrypted and checked."""
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


def fmt(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} - {max(v):.2f})"


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    count, W, W2 = 4096, ol.n + 1, ol.N2 + 1
    L = ol.load()
    keys = ol.Keys(L, seed=1)
    keys2 = ol.KeysLvl2(L, keys, seed=7)
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    eng.lvl2_initialize(keys2.bk, keys2.ksk)
    print(f"device: {api.device_identity()}  cus: {api.device_cus()}\n")
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2, size=(2, count)).astype(np.uint8)
    a = api.DeviceBuffer(count * W).upload(keys.encrypt(bits[0], 0, seed=1))
    b = api.DeviceBuffer(count * W).upload(keys.encrypt(bits[1], 0, seed=2))
    out = api.DeviceBuffer(count * W)
    t2 = api.DeviceBuffer(count * W2 * 2)
    # NAND as a table on the sum: x = -a - b + mu has phase -1/8, 1/8 or 3/8; the table of p = 8 boxes that holds mu everywhere is the
    # built-in gate's constant test vector except in the top half-box (phases within 1/32 of 1/2, far from 3/8), which holds -mu
    f = np.array([1, 1, 1, 1, 1, 1, 1, 1], np.uint64) * np.uint64(ol.MU2)
    tv = eng.lvl2_test_vector(f)
    nand_plain = eng.lvl2_define_gate((-1, -1, 0), ol.MU)
    nand_table = eng.lvl2_define_gate((-1, -1, 0), ol.MU, tv)
    runs = {
        "NAND (built-in)": lambda: eng.lvl2_gate_batch(api.NAND, out, a, b, count=count),
        "lvl2 user gate, NAND numbers, no TV": lambda: eng.lvl2_gate_batch(nand_plain, out, a, b, count=count),
        "lvl2 user gate, NAND numbers, table TV": lambda: eng.lvl2_gate_batch(nand_table, out, a, b, count=count),
        "the table gate without its key switch": lambda: eng.lvl2_user_extract_batch(nand_table, a, t2, count, in1=b),
    }
    t = {k: [] for k in runs}
    for f_run in runs.values():          # warm-up
        f_run()
    eng.Synchronize()
    for _ in range(reps):
        for name, f_run in runs.items():
            t0 = time.perf_counter()
            f_run()
            eng.Synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3)
    print("## 4096-gate batch on the N = 2048 ring (ms per batch: median (min - max) over", reps, "alternated repetitions)\n")
    print("| gate | ms |\n|---|---|")
    for k, v in t.items():
        print(f"| {k} | {fmt(v)} |")
    eng.lvl2_gate_batch(nand_table, out, a, b, count=count)
    eng.Synchronize()
    ok = list(keys.decrypt(out.download().reshape(count, W), 0)) == list(1 - bits[0] * bits[1])
    print(f"\nall table gates decrypted to NAND: {ok}")
    eng.CleanUp()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
