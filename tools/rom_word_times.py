"""Packed ROM words on the GPU (profiles/r11_packed_rom.md).  One process, count = 4096 items per launch
(argv[1]), warm-up then the median of argv[2] = 20 alternating repetitions, host clock around launches that end in Synchronize:
  - the rotating CMUX against cufhe_amd_trlwe_rotate_batch followed by cufhe_amd_cmux_batch (the same words, one buffer more);
  - cufhe_amd_cmux_batch, the indexed extraction + key switch and the extraction at 0 + key switch;
  - from these per-item times, one read of a 256-entry ROM of 8-bit words as 8 single-bit trees (8 x 255 CMUX + 8 extractions) and
    packed into 2 TRLWEs x 128 words (7 rotating CMUX on each + 1 CMUX + 8 indexed extractions): priced, not run as one program.
Operands are random words: timing does not depend on them.  Usage: python tools/rom_word_times.py [count] [reps]"""
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

api, N, n = eng.api, ol.N, ol.n


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    keys = ol.Keys(ol.load(), seed=1)
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    rng = np.random.default_rng(11)
    words = lambda k: rng.integers(0, 2**32, size=k, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    c, trgsw = api.DeviceBuffer(count * 2 * N).upload(words(count * 2 * N)), api.DeviceBuffer(12 * N).upload(words(12 * N))
    ntt1, nttc = api.DeviceBuffer(24 * N), api.DeviceBuffer(count * 24 * N)
    api.trgsw_to_ntt_batch(trgsw, ntt1, 1)
    eng.Synchronize()
    nttc.upload(np.tile(ntt1.download(), count))     # one copy of the selector per item for cufhe_amd_cmux_batch
    rot, res, t0 = api.DeviceBuffer(count * 2 * N), api.DeviceBuffer(count * 2 * N), api.DeviceBuffer(count * (n + 1))
    e = rng.integers(0, 2 * N, size=count).astype(np.int32)
    j = rng.integers(0, N, size=count).astype(np.int32)
    runs = {"cmux_rotate_batch": lambda: api.cmux_rotate_batch(ntt1, e, c, res, count),
            "trlwe_rotate_batch + cmux_batch": lambda: (api.trlwe_rotate_batch(c, e, rot, count), api.cmux_batch(nttc, rot, c, res, count)),
            "cmux_batch": lambda: api.cmux_batch(nttc, rot, c, res, count),
            "sample_extract_index_keyswitch_batch": lambda: api.sample_extract_index_keyswitch_batch(c, j, t0, count),
            "sample_extract_keyswitch_batch": lambda: api.sample_extract_keyswitch_batch(c, t0, count)}
    ms = {k: [] for k in runs}
    for r in range(reps + 2):                    # two warm-up rounds; the candidates alternate inside a round
        for k, f in runs.items():
            eng.Synchronize()
            t = time.perf_counter()
            f()
            eng.Synchronize()
            if r >= 2:
                ms[k].append((time.perf_counter() - t) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(f"count {count}, {reps} repetitions, {eng.device_identity(0)}, clock {api.probe_clock(0) / 1e6:.0f} MHz")
    print("| launch | median ms | min | max | us / item |")
    print("|---|---|---|---|---|")
    for k, v in ms.items():
        print(f"| {k} | {med[k]:.3f} | {min(v):.3f} | {max(v):.3f} | {med[k] * 1e3 / count:.3f} |")
    per = {k: med[k] * 1e3 / count for k in med}
    trees = 8 * 255 * per["cmux_batch"] + 8 * per["sample_extract_keyswitch_batch"]
    packed = 14 * per["cmux_rotate_batch"] + per["cmux_batch"] + 8 * per["sample_extract_index_keyswitch_batch"]
    print(f"one 8-bit read of 256 entries, priced per item at this count: 8 single-bit trees {trees:.1f} us, packed {packed:.1f} us ({trees / packed:.1f}x)")
    eng.CleanUp()


if __name__ == "__main__":
    main()
