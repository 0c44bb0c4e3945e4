"""Linear layers by shape: cufhe_amd_linear_batch alone, cufhe_amd_linear_gate_batch, and cufhe_amd_gate_batch of the same number of
one-input user gates -- the difference of the last two is what the layer adds to the bootstraps it feeds -- beside the key-switch
launch of a 4096 batch.  Device-resident operands, event-timed on the stream the calls run on, the variants alternated inside every
repetition of one process.  Level 0.  python tools/linear_times.py [reps]"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch
import cufhe_amd as eng

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
SHAPES = ((64, 64, 64), (1024, 1024, 4), (4096, 4096, 1))          # (rows, cols, sets)
rng = np.random.default_rng(27)
P = eng.PARAMS
bk = rng.integers(0, 2**32, size=int(P.bk_words), dtype=np.uint64).astype(np.uint32)
ksk = rng.integers(0, 2**32, size=int(P.ksk_words), dtype=np.uint64).astype(np.uint32)
eng.SetGPUNum(1)
eng.Initialize(bk, ksk)
words, N = int(P.n) + 1, int(P.N)
op = eng.define_gate((1, 0, 0), 0, rng.integers(0, 2**32, size=N, dtype=np.uint64).astype(np.uint32))


def words_of(count):
    return rng.integers(0, 2**32, size=count * words, dtype=np.uint64).astype(np.uint32)


def timed(fn):
    """ms of one call on the null stream, between two events recorded on it"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


ks_in = eng.api.DeviceBuffer(4096 * (N + 1)).upload(rng.integers(0, 2**32, size=4096 * (N + 1), dtype=np.uint64).astype(np.uint32))
ks_out = eng.api.DeviceBuffer(4096 * words)
rows_out = []
for rows, cols, sets in SHAPES:
    W = rng.integers(-(1 << 31), 1 << 31, size=(rows, cols), dtype=np.int64)
    layer = eng.define_linear(W, rng.integers(0, 2**32, size=rows, dtype=np.uint64))
    din = eng.api.DeviceBuffer(sets * cols * words).upload(words_of(sets * cols))
    dsum, dfused, dgate = (eng.api.DeviceBuffer(sets * rows * words) for _ in range(3))
    count = sets * rows
    variants = {
        "linear": lambda: eng.linear_batch(layer, 0, dsum, din, sets),
        "fused": lambda: eng.linear_gate_batch(layer, op, 0, dfused, din, sets),
        "gates": lambda: eng.gate_batch(op, 0, dgate, dsum, count=count),
        "keyswitch4096": lambda: eng.api.keyswitch_batch(ks_in, ks_out, 4096),
    }
    for fn in variants.values():          # warm: workspaces, the pooled temporary, code objects
        fn()
    eng.Synchronize()
    t = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t[k].append(timed(fn))
    same = bool(np.array_equal(dfused.download(), dgate.download()))          # the gates ran on the linear call's sums
    r = {"rows": rows, "cols": cols, "sets": sets, "gates": count, "fused_equals_composition": same}
    for k, v in t.items():
        v.sort()
        r[k] = {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}
    r["added_fraction"] = (r["fused"]["median"] - r["gates"]["median"]) / r["gates"]["median"]
    r["linear_over_keyswitch4096"] = r["linear"]["median"] / r["keyswitch4096"]["median"]
    rows_out.append(r)
    print(f"{rows:5d} x {cols:5d} x {sets:3d}  linear {r['linear']['min']:.4f} / {r['linear']['median']:.4f} / {r['linear']['max']:.4f}   "
          f"fused {r['fused']['median']:.3f}   gates {r['gates']['median']:.3f}   key switch of 4096 {r['keyswitch4096']['median']:.4f} ms "
          f"(min / median / max of {reps})   added {100 * r['added_fraction']:.2f} %   linear / key switch {r['linear_over_keyswitch4096']:.2f}   "
          f"fused == linear then gates: {same}", flush=True)
print(json.dumps({"linear_times": rows_out}))
eng.CleanUp()
