"""Recorded lookups against the other ways to issue the same work (profiles/r23_recorded_lookups.md).  One process alternates
  - batch     4096 lookups as ONE cufhe_amd_lut_lookup_batch on device arrays,
  - recorded  4096 recorded lookups through the per-gate API on device buffers (gLookup, 8 streams), then Synchronize(),
  - nand      4096 recorded NANDs the same way (gNand): the yardstick the per-gate API already has,
  - blocking  64 blocking gLookupTRLWE calls (fence, allocation, count = 1 launches, stream synchronisation): enough to price one.
Two warm-up rounds, then `rounds` rounds that run the four in turn; wall time per candidate, median / min / max, items per second
from the median.  After the last round the scheduler's statistics and timeline of one recorded-lookup run are printed
(cufhe_amd_sched_get_stats / _get_trace).  Inputs are random words: the times do not depend on them.
Usage: python tools/recorded_lookup_times.py [rounds]"""
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
COUNT, BLOCKING, STREAMS, TABLES = 4096, 64, 8, 16


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    keys = ol.Keys(ol.load(), seed=1)
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    n, N = api.PARAMS.n, api.PARAMS.N
    rng = np.random.default_rng(1)
    x = rng.integers(0, 2**32, size=(COUNT, n + 1), dtype=np.uint32)
    t = rng.integers(0, 2**32, size=(TABLES, 2 * N), dtype=np.uint32)
    src = (np.arange(COUNT) % TABLES).astype(np.int32)
    dx, dt, dout = api.DeviceBuffer(x.size).upload(x), api.DeviceBuffer(t.size).upload(t), api.DeviceBuffer(COUNT * (n + 1))
    streams = []
    for _ in range(STREAMS):
        s = api.Stream()
        s.Create()
        streams.append(s)
    tabs = []
    for k in range(TABLES):
        h = api.Trlwe()
        h.trlwehost[:] = t[k]
        api.CtxtCopyH2D(h, streams[0])
        tabs.append(h)
    a, b, o = [], [], []
    for g in range(COUNT):
        for lst, words in ((a, x[g]), (b, x[(g + 1) % COUNT]), (o, x[g])):
            c = api.Ctxt(0)
            c.tlwehost[:] = words
            api.CtxtCopyH2D(c, streams[g % STREAMS])
            lst.append(c)
    eng.Synchronize()
    op = api.DefineLookup((1, 0), 0, 1)

    def batch():
        api.lut_lookup_batch(dx, dt, dout, COUNT, TABLES, src=src)
        eng.Synchronize()
        return COUNT

    def recorded():
        for g in range(COUNT):
            api.gLookup([o[g]], tabs[g % TABLES], a[g], None, op, streams[g % STREAMS])
        eng.Synchronize()
        return COUNT

    def nand():
        for g in range(COUNT):
            api.gNand(o[g], a[g], b[g], streams[g % STREAMS])
        eng.Synchronize()
        return COUNT

    def blocking():
        for g in range(BLOCKING):
            api.gLookupTRLWE([o[g]], tabs[g % TABLES], a[g], streams[0])
        eng.Synchronize()
        return BLOCKING

    candidates = (("batch", batch), ("recorded", recorded), ("nand", nand), ("blocking", blocking))
    for _ in range(2):
        for _, fn in candidates:
            fn()
    times = {name: [] for name, _ in candidates}
    items = {}
    for _ in range(rounds):
        for name, fn in candidates:
            t0 = time.perf_counter()
            items[name] = fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    print(f"device: {api.device_cus()} CUs; {rounds} rounds after 2 warm-up rounds; wall ms per call sequence, Synchronize() included")
    print("| candidate | items | median ms | min ms | max ms | items / s (median) | us / item |")
    print("|---|---:|---:|---:|---:|---:|---:|")
    for name, _ in candidates:
        v = times[name]
        med = statistics.median(v)
        print(f"| {name} | {items[name]} | {med:.3f} | {min(v):.3f} | {max(v):.3f} | {items[name] / med * 1e3:.0f} | {med / items[name] * 1e3:.2f} |")
    api.sched_stats(reset=True)
    api.sched_trace(clear=True)
    api.profile_enable(True)
    recorded()
    s = api.sched_stats()
    print(f"\none recorded run: gates {s.gates}, flushes {s.groups}, levels {s.levels}, launch sequences {s.launch_sequences}, "
          f"record {s.record_ns / 1e6:.3f} ms, launch {s.launch_ns / 1e6:.3f} ms, retire {s.retire_ns / 1e6:.3f} ms")
    for row in api.sched_trace(clear=True):
        print("  ", row)
    api.profile_enable(False)
    eng.CleanUp()


if __name__ == "__main__":
    main()
