"""TLWE packing on the GPU (profiles/r12_tlwe_packing.md).  One process:
  - cufhe_amd_pack_batch at 8, 64 and 4096 inputs (one output per 8 inputs, positions 0 .. 7): the kernel's time from the library's
    profiling events (cufhe_amd_profile_get: keyswitch_ms, the HIP events around the launch), median over the repetitions, the wall
    time per call beside it, the launch shape (tiles x slices), the bytes of the key sweep -- every tile reads the whole key once
    -- and the bandwidth that makes;
  - cufhe_amd_private_keyswitch_batch at the same input counts, measured the same way in the same process, and the ratio of the
    per-input times against the ratio of the (i, j) pairs visited: packing 630 x 8 = 5 040 pairs of 3 candidate rows, the private
    key switch 2 x 2049 x 10 = 40 980 of 7.
Both keys are random words: timing does not depend on them.  PACK_ONLY=1 skips the private key switch (its key is 2.35 GB).
Usage: python tools/pack_times.py [reps]"""
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
COUNTS = (8, 64, 4096)
TILE, CHUNKS, I_BLOCK = 64, 8, 16          # kernels_pack.hip.h


def timed(run, reps):
    """(median kernel ms from the profiling events, median wall ms) of run()"""
    run()
    eng.Synchronize()
    ev, wall = [], []
    for _ in range(reps):
        api.profile_enable(True)
        api.profile_get(reset=True)
        t0 = time.perf_counter()
        run()
        eng.Synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(api.profile_get(reset=True).keyswitch_ms)
        api.profile_enable(False)
    return statistics.median(ev), statistics.median(wall)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    L = ol.load()
    keys = ol.Keys(L, seed=1)
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    cus = api.device_cus()
    p = api.pack_params()
    rng = np.random.default_rng(1)
    api.pack_initialize(rng.integers(0, 2**32, size=p.key_words, dtype=np.uint32))
    key_bytes = p.key_words * 4
    pack = {}
    print(f"device: {cus} CUs; packing key {key_bytes / 1e6:.1f} MB")
    print("| inputs | tiles x slices | kernel ms | wall ms | us / input | key sweep MB | GB/s |")
    print("|---:|---:|---:|---:|---:|---:|---:|")
    for count in COUNTS:
        x = rng.integers(0, 2**32, size=count * (p.n + 1), dtype=np.uint32)
        d0 = api.DeviceBuffer(x.size).upload(x)
        count_out = (count + 7) // 8
        dt = api.DeviceBuffer(count_out * 2 * p.N)
        dst, pos = np.arange(count, dtype=np.int32) // 8, np.arange(count, dtype=np.int32) % 8
        ms, wall = timed(lambda: api.pack_batch(d0, dst, pos, dt, count, count_out), reps)
        tiles = (count + TILE - 1) // TILE
        wgs = tiles * CHUNKS
        slices = 1 if wgs >= 4 * cus else min((p.n + I_BLOCK - 1) // I_BLOCK, -(-4 * cus // wgs))      # plan::plan_pack
        sweep = tiles * key_bytes
        pack[count] = ms
        print(f"| {count} | {tiles} x {slices} | {ms:.4f} | {wall:.4f} | {ms / count * 1e3:.3f} | {sweep / 1e6:.0f} | {sweep / ms / 1e6:.0f} |")
        del d0, dt
    if os.environ.get("PACK_ONLY") == "1":
        return
    cb = api.cb_params()
    api.cb_initialize(rng.integers(0, 2**32, size=cb.privksk_words, dtype=np.uint32))
    print()
    print("| inputs | private key switch kernel ms | us / input | packing us / input | ratio | pairs ratio 5040 / 40980 | ratio / pairs ratio |")
    print("|---:|---:|---:|---:|---:|---:|---:|")
    pairs = 5040 / 40980
    for count in COUNTS:
        x = rng.integers(0, 2**32, size=count * cb.lvl2_words * 2, dtype=np.uint32)
        d2 = api.DeviceBuffer(x.size).upload(x)
        dt = api.DeviceBuffer(count * 2 * 2 * cb.N)
        ms, _ = timed(lambda: api.private_keyswitch_batch(d2, dt, count), reps)
        ratio = (pack[count] / count) / (ms / count)
        print(f"| {count} | {ms:.4f} | {ms / count * 1e3:.3f} | {pack[count] / count * 1e3:.3f} | {ratio:.4f} | {pairs:.4f} | {ratio / pairs:.3f} |")
        del d2, dt


if __name__ == "__main__":
    main()
