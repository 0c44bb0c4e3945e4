"""Recorded packs against the other ways to issue the same work (profiles/r24_recorded_pack.md).  One process alternates
  - recorded  64 packs of 8 gate results each, recorded with gPack behind the 512 recorded NANDs that produce them, then Synchronize(),
  - blocking  the same 512 NANDs and 64 blocking gPackTLWEs calls (fence, gather allocation, Copy launch, a one-output pack, stream
              synchronisation each), then Synchronize(),
  - batch     ONE cufhe_amd_pack_batch of 512 pre-gathered inputs into 64 outputs on device arrays, then Synchronize(): the floor (no
              gates: the packing alone),
  - gates     the 512 recorded NANDs alone, then Synchronize(): what the first two spend outside packing.
Two warm-up rounds, then `rounds` rounds that run the four in turn; wall time per candidate, median / min / max.  After the last round
the scheduler's statistics and the profiled launcher calls of one recorded run are printed.  The key and the inputs are random words: the
times do not depend on them.
Usage: python tools/recorded_pack_times.py [rounds]"""
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
PACKS, ARITY, STREAMS = 64, 8, 8
GATES = PACKS * ARITY


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    keys = ol.Keys(ol.load(), seed=1)
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    n, N = api.PARAMS.n, api.PARAMS.N
    rng = np.random.default_rng(1)
    api.pack_initialize(rng.integers(0, 2**32, size=int(api.pack_params().key_words), dtype=np.uint32))
    x = rng.integers(0, 2**32, size=(GATES, n + 1), dtype=np.uint32)
    dx, dout = api.DeviceBuffer(x.size).upload(x), api.DeviceBuffer(PACKS * 2 * N)
    dst = (np.arange(GATES) // ARITY).astype(np.int32)
    pos = (np.arange(GATES) % ARITY).astype(np.int32)
    streams = []
    for _ in range(STREAMS):
        s = api.Stream()
        s.Create()
        streams.append(s)
    a, b, o = [], [], []
    for g in range(GATES):
        for lst, words in ((a, x[g]), (b, x[(g + 1) % GATES]), (o, x[g])):
            c = api.Ctxt(0)
            c.tlwehost[:] = words
            api.CtxtCopyH2D(c, streams[g % STREAMS])
            lst.append(c)
    words = [api.Trlwe() for _ in range(PACKS)]
    eng.Synchronize()
    positions = list(range(ARITY))

    def gates():
        for g in range(GATES):
            api.gNand(o[g], a[g], b[g], streams[g % STREAMS])

    def recorded():
        gates()
        for k in range(PACKS):
            api.gPack(words[k], o[k * ARITY:(k + 1) * ARITY], positions, streams[k % STREAMS])
        eng.Synchronize()

    def blocking():
        gates()
        for k in range(PACKS):
            api.gPackTLWEs(words[k], o[k * ARITY:(k + 1) * ARITY], positions, streams[k % STREAMS])
        eng.Synchronize()

    def batch():
        api.pack_batch(dx, dst, pos, dout, GATES, PACKS)
        eng.Synchronize()

    def gates_alone():
        gates()
        eng.Synchronize()

    candidates = (("recorded", recorded), ("blocking", blocking), ("batch", batch), ("gates", gates_alone))
    for _ in range(2):
        for _, fn in candidates:
            fn()
    times = {name: [] for name, _ in candidates}
    for _ in range(rounds):
        for name, fn in candidates:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    print(f"device: {api.device_cus()} CUs; {PACKS} packs of {ARITY}; {rounds} rounds after 2 warm-up rounds; wall ms, Synchronize() included")
    print("| candidate | median ms | min ms | max ms |")
    print("|---|---:|---:|---:|")
    for name, _ in candidates:
        v = times[name]
        print(f"| {name} | {statistics.median(v):.3f} | {min(v):.3f} | {max(v):.3f} |")
    api.sched_stats(reset=True)
    api.profile_enable(True)
    api.profile_get(reset=True)
    recorded()
    s = api.sched_stats()
    p = api.profile_get(reset=True)
    api.profile_enable(False)
    print(f"\none recorded run: gates {s.gates}, flushes {s.groups}, levels {s.levels}, launch sequences {s.launch_sequences}, "
          f"record {s.record_ns / 1e6:.3f} ms, launch {s.launch_ns / 1e6:.3f} ms, retire {s.retire_ns / 1e6:.3f} ms; "
          f"profiled launcher calls: rotations {p.blind_rotate_launches} ({p.blind_rotations} units), "
          f"key switches and packs {p.keyswitch_launches} ({p.keyswitches} units)")
    eng.CleanUp()


if __name__ == "__main__":
    main()
