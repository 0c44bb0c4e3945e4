"""Encrypted-table lookups on the GPU (profiles/r13_encrypted_lut.md).  One process:
  - cufhe_amd_lut_lookup_batch (nout = 1, every item its own table) at 8, 256 and 4096 items against cufhe_amd_bootstrap_batch at the
    same counts: wall time per call (stream-synchronised, median over the repetitions) and the kernel times of the library's
    profiling events (blind rotation and key switch separately), lookups per second from the wall time;
  - cufhe_amd_trlwe_spread_batch (stride 1, reps 256) alone at 1, 64 and 4096 TRLWEs: wall time per call.
Tables, keys' inputs and TRLWEs are random words: the times do not depend on them.
Usage: python tools/lut_times.py [reps]"""
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
COUNTS = (8, 256, 4096)
SPREAD_COUNTS = (1, 64, 4096)


def timed(run, reps):
    """medians of (wall ms, blind-rotate kernel ms, key-switch kernel ms) of run()"""
    run()
    eng.Synchronize()
    wall, br, ks = [], [], []
    for _ in range(reps):
        api.profile_enable(True)
        api.profile_get(reset=True)
        t0 = time.perf_counter()
        run()
        eng.Synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        p = api.profile_get(reset=True)
        br.append(p.blind_rotate_ms)
        ks.append(p.keyswitch_ms)
        api.profile_enable(False)
    return statistics.median(wall), statistics.median(br), statistics.median(ks)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    keys = ol.Keys(ol.load(), seed=1)
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    n, N = api.PARAMS.n, api.PARAMS.N
    rng = np.random.default_rng(1)
    print(f"device: {api.device_cus()} CUs; {reps} repetitions")
    print("| items | lookup wall ms | rotation ms | key switch ms | lookups / s | bootstrap wall ms | rotation ms | key switch ms | bootstraps / s | lookup / bootstrap wall |")
    print("|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    for count in COUNTS:
        dx = api.DeviceBuffer(count * (n + 1)).upload(rng.integers(0, 2**32, size=count * (n + 1), dtype=np.uint32))
        dt = api.DeviceBuffer(count * 2 * N).upload(rng.integers(0, 2**32, size=count * 2 * N, dtype=np.uint32))
        dout = api.DeviceBuffer(count * (n + 1))
        lw, lb, lk = timed(lambda: api.lut_lookup_batch(dx, dt, dout, count, count), reps)
        bw, bb, bk = timed(lambda: api.bootstrap_batch(dout, dx, count), reps)
        print(f"| {count} | {lw:.4f} | {lb:.4f} | {lk:.4f} | {count / lw * 1e3:.0f} | {bw:.4f} | {bb:.4f} | {bk:.4f} | {count / bw * 1e3:.0f} | {lw / bw:.4f} |")
        del dx, dt, dout
    print()
    print("| TRLWEs | spread wall ms | us / TRLWE | GB/s (read + write) |")
    print("|---:|---:|---:|---:|")
    for count in SPREAD_COUNTS:
        din = api.DeviceBuffer(count * 2 * N).upload(rng.integers(0, 2**32, size=count * 2 * N, dtype=np.uint32))
        dout = api.DeviceBuffer(count * 2 * N)
        w, _, _ = timed(lambda: api.trlwe_spread_batch(din, dout, count, 1, 256), reps)
        print(f"| {count} | {w:.4f} | {w / count * 1e3:.3f} | {2 * count * 2 * N * 4 / w / 1e6:.1f} |")
        del din, dout


if __name__ == "__main__":
    main()
