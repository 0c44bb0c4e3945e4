"""The lvl10 key switch by launch size: the kernels of the default rule ("ks_mm_threshold" 0) against the matrix-product kernel
("ks_mm_threshold" 1), HIP-event time of the whole launcher call (digit pre-pass included), per repetition; the outputs of the two
are compared word for word at every count.  python tools/ks_mm_times.py [reps]"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch  # noqa: F401
import cufhe_amd as eng

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 11
rng = np.random.default_rng(1)
P = eng.PARAMS
bk = rng.integers(0, 2**32, size=int(P.bk_words), dtype=np.uint64).astype(np.uint32)
ksk = rng.integers(0, 2**32, size=int(P.ksk_words), dtype=np.uint64).astype(np.uint32)
eng.SetGPUNum(1)
eng.Initialize(bk, ksk)
n, N = int(P.n), int(P.N)
mx = 4096
a = rng.integers(0, 2**32, size=(mx, N + 1), dtype=np.uint64).astype(np.uint32)
d1 = eng.api.DeviceBuffer(a.size)
d1.upload(a)
d0 = eng.api.DeviceBuffer(mx * (n + 1))


def times(count):
    eng.api.keyswitch_batch(d1, d0, count)      # warm: workspace, code objects
    eng.Synchronize()
    out = []
    for _ in range(reps):
        eng.api.profile_enable(True)
        eng.api.profile_get(reset=True)
        eng.api.keyswitch_batch(d1, d0, count)
        eng.Synchronize()
        out.append(eng.api.profile_get(reset=True).keyswitch_ms)
    eng.api.profile_enable(False)
    return sorted(out)


rows = []
for count in (64, 128, 256, 512, 1024, 1536, 2048, 3072, 4096):
    r = {"count": count}
    words = {}
    for name, thr in (("rule", 0), ("matrix", 1)):
        eng.api.set_option("ks_mm_threshold", thr)
        t = times(count)
        r[name] = {"min": t[0], "median": t[len(t) // 2], "max": t[-1]}
        words[name] = d0.download()[:count * (n + 1)].copy()
    r["same_words"] = bool(np.array_equal(words["rule"], words["matrix"]))
    rows.append(r)
    print(f"{count:5d}  rule {r['rule']['min']:.4f} / {r['rule']['median']:.4f} / {r['rule']['max']:.4f}   "
          f"matrix {r['matrix']['min']:.4f} / {r['matrix']['median']:.4f} / {r['matrix']['max']:.4f} ms (min / median / max of {reps})   "
          f"same words: {r['same_words']}", flush=True)
eng.api.set_option("ks_mm_threshold", -1)
print(json.dumps({"ks_mm_times": rows}))
eng.CleanUp()
