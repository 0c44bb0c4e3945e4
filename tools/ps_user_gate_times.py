"""User gates of the compiled parameter sets against the sets' built-in NAND on the GPU (profiles/r20_ps_user_gates.md).  One process;
per set, runs alternated:
  - 4096 NAND through cufhe_amd_ps_gate_batch (pad 0: the +-mu compare-select of the rotation kernels),
  - 4096 single-output table gates (cufhe_amd_ps_test_vector, p = 4: R gathered words per lane before the n steps),
  - 4096 two-output gates, both outputs requested (8192 list entries through cufhe_amd_gate_list while "param_set" is the set: the
    outputs of one evaluation share the rotation; two key switches per evaluation)
-- ms per batch over the repetitions, timed from the call to the end of cufhe_amd_synchronize.  Prints a markdown table per set.  Keys
and ciphertexts come from the set's CPU oracle (seeded); the table gate's outputs are decrypted and checked.
   python tools/ps_user_gate_times.py [repetitions]"""
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

api = eng.api


def fmt(v):
    return f"{statistics.median(v):.2f} ({min(v):.2f} - {max(v):.2f})"


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    count = 4096
    eng.SetGPUNum(1)
    eng.Initialize()
    print(f"device: {api.device_identity()}  cus: {api.device_cus()}\n")
    ok_all = True
    for name in ol.SETS:
        K = ol.Keys(ol.load_set(name), seed=5)
        ps = api.ps_index(name)
        api.ps_initialize(ps, K.bk, K.ksk)
        W = K.words[0]
        rng = np.random.default_rng(7)
        bits = rng.integers(0, 2, size=(2, count)).astype(np.uint8)
        a = api.DeviceBuffer(count * W).upload(K.encrypt(bits[0], 0, seed=1))
        b = api.DeviceBuffer(count * W).upload(K.encrypt(bits[1], 0, seed=2))
        out = api.DeviceBuffer(2 * count * W)
        # NAND as a table on the sum: x = -a - b + mu has phase -1/8, 1/8 or 3/8; p = 4 boxes that hold mu everywhere are the built-in
        # gate's constant test vector except in the top half-box (phases within 1/16 of 1/2), which holds -mu
        mu = np.full(4, ol.MU, np.uint32)
        table = api.ps_define_gate(ps, (-1, -1, 0), ol.MU, api.ps_test_vector(ps, mu))
        two = api.ps_define_gate(ps, (-1, -1, 0), ol.MU, api.ps_test_vector_multi(ps, [mu, (0 - mu.astype(np.int64)).astype(np.uint32)]), nout=2)
        ops2 = np.array([api.ps_user_op_output(two, g % 2) for g in range(2 * count)], np.int32)
        ptrs = lambda buf, rep: (ctypes.c_void_p * (2 * count))(*[buf.ptr + 4 * W * (g // rep) for g in range(2 * count)])  # noqa: E731
        outs, in0s, in1s = ptrs(out, 1), ptrs(a, 2), ptrs(b, 2)

        def run_two():
            api.set_option("param_set", ps)
            try:
                eng.check(eng.lib.cufhe_amd_gate_list(0, None, 0, 2 * count, ops2.ctypes.data, outs, in0s, in1s, None))
            finally:
                api.set_option("param_set", -1)
        runs = {
            "NAND (built-in)": lambda: api.ps_gate_batch(ps, api.NAND, out, a, b, count=count),
            "table gate, p = 4": lambda: api.ps_gate_batch(ps, table, out, a, b, count=count),
            "two-output gate, both outputs": run_two,
        }
        t = {k: [] for k in runs}
        for f_run in runs.values():          # warm-up
            f_run()
        eng.Synchronize()
        for _ in range(reps):
            for k, f_run in runs.items():
                t0 = time.perf_counter()
                f_run()
                eng.Synchronize()
                t[k].append((time.perf_counter() - t0) * 1e3)
        print(f"## {name}: 4096 gates per batch (ms per batch: median (min - max) over {reps} alternated repetitions)\n")
        print("| gate | ms |\n|---|---|")
        for k, v in t.items():
            print(f"| {k} | {fmt(v)} |")
        api.ps_gate_batch(ps, table, out, a, b, count=count)
        eng.Synchronize()
        ok = list(K.decrypt(out.download(count * W).reshape(count, W), 0)) == list(1 - bits[0] * bits[1])
        run_two()
        eng.Synchronize()
        both = out.download().reshape(count, 2, W)
        ok2 = list(K.decrypt(both[:, 0], 0)) == list(1 - bits[0] * bits[1]) and list(K.decrypt(both[:, 1], 0)) == list(bits[0] * bits[1])
        print(f"\nall table gates decrypted to NAND: {ok}; two-output gates to (NAND, AND): {ok2}\n", flush=True)
        ok_all = ok_all and ok and ok2
        for buf in (a, b, out):
            buf.free()
    eng.CleanUp()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
