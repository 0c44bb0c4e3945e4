"""Two-output gates of the N = 2048 ring against pairs of single-output gates on the GPU (profiles/r18_lvl2_multi_output.md).  One
process, runs alternated: 8192 lvl0 outputs -- sum and carry of 4096 full adders, bits as padded p = 4 messages b / 8 -- through
cufhe_amd_gate_list with "lvl0_ring" 2048, as
  - 4096 evaluations of ONE 2-output definition (sum and carry name the same operands: 4096 rotations, 8192 key switches),
  - 4096 + 4096 single-output gates (a sum table and a carry table: 8192 rotations, 8192 key switches)
-- ms per list over the repetitions, and the rotation / key-switch split of the library's profiling events.  Prints a markdown table.
Keys and ciphertexts come from the CPU oracle (seeded); both forms' outputs are decrypted and checked."""
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
import oracle_lib as ol  # noqa: E402
import user_gate_checker as uc  # noqa: E402

api = eng.api
EIGHTH = 1 << 61


def fmt(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} - {max(v):.2f})"


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    evals, W = 4096, ol.n + 1
    L = ol.load()
    keys = ol.Keys(L, seed=1)
    keys2 = ol.KeysLvl2(L, keys, seed=7)
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    eng.lvl2_initialize(keys2.bk, keys2.ksk)
    api.set_option("lvl0_ring", 2048)
    print(f"device: {api.device_identity()}  cus: {api.device_cus()}\n")
    rng = np.random.default_rng(7)
    bits = rng.integers(0, 2, size=(3, evals))
    d = [api.DeviceBuffer(evals * W).upload(uc.encrypt_torus(keys, 0, bits[k].astype(np.uint64) * np.uint64(1 << 29), 2.0 ** 17, seed=k + 1))
         for k in range(3)]
    out = api.DeviceBuffer(2 * evals * W)
    vals = np.array([[(m & 1) * EIGHTH for m in range(4)], [(m >> 1) * EIGHTH for m in range(4)]], np.uint64)
    multi = eng.lvl2_define_gate((1, 1, 1), 0, eng.lvl2_test_vector_multi(vals), nout=2)
    single = [eng.lvl2_define_gate((1, 1, 1), 0, eng.lvl2_test_vector(vals[j])) for j in range(2)]
    arr = lambda ps: (ctypes.c_void_p * len(ps))(*ps)  # noqa: E731
    # gate 2 g + j: output j of evaluation g
    outs = arr([out.ptr + 4 * W * i for i in range(2 * evals)])
    ins = [arr([d[k].ptr + 4 * W * (i // 2) for i in range(2 * evals)]) for k in range(3)]
    ops = {"one 2-output gate per evaluation": np.array([eng.lvl2_user_op_output(multi, i % 2) for i in range(2 * evals)], np.int32),
           "two single-output gates per evaluation": np.array([single[i % 2] for i in range(2 * evals)], np.int32)}

    def run(name):
        eng.check(eng.lib.cufhe_amd_gate_list(0, None, 0, 2 * evals, ops[name].ctypes.data, outs, ins[0], ins[1], ins[2]))

    ok = True
    x = bits.sum(axis=0)
    want = np.stack([x & 1, x >> 1], axis=1).reshape(-1)
    for name in ops:                     # warm-up, and the decrypt check of both forms
        run(name)
        eng.Synchronize()
        ph = uc.phase(keys, 0, out.download().reshape(2 * evals, W)).astype(np.int64)
        ok &= bool(np.array_equal(np.rint(ph / float(1 << 29)).astype(np.int64) % 8, want))
    t, br, ks, nrot = ({k: [] for k in ops} for _ in range(4))
    for _ in range(reps):
        for name in ops:
            api.profile_enable(True)
            api.profile_get(reset=True)
            t0 = time.perf_counter()
            run(name)
            eng.Synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3)
            p = api.profile_get(reset=True)
            api.profile_enable(False)
            br[name].append(p.blind_rotate_ms)
            ks[name].append(p.keyswitch_ms)
            nrot[name].append(p.blind_rotations)
    print(f"## {2 * evals} outputs on the N = 2048 ring (ms per list: median (min - max) over {reps} alternated repetitions)\n")
    print("| form | rotations | ms | rotations ms | key switches ms |\n|---|---:|---|---|---|")
    for k in ops:
        print(f"| {k} | {nrot[k][0]} | {fmt(t[k])} | {fmt(br[k])} | {fmt(ks[k])} |")
    a, b = (statistics.median(t[k]) for k in ops)
    print(f"\ntwo single-output gates / one 2-output gate: {b / a:.2f}x")
    print(f"all outputs of both forms decrypted to sum and carry: {ok}")
    api.set_option("lvl0_ring", 1024)
    eng.CleanUp()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
