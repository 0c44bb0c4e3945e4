"""Circuit bootstrapping on the GPU (profiles/r09_circuit_bootstrapping.md, profiles/r18_lvl2_multi_output.md).  One process:
  - CB/s of cufhe_amd_circuit_bootstrap_batch (NTT-domain output) at 1, 8, 64, 512 and 4096 inputs, in BOTH forms -- three rotations
    per input ("cb_rotations" 3, the default) and one ("cb_rotations" 1) -- alternated repetition by repetition in the same run: wall
    time per batch (median over the repetitions, Synchronize around each) and its split into the lvl02 rotations / the private key
    switch from the library's profiling events (cufhe_amd_profile_get: blind_rotate_ms = rotations, keyswitch_ms = private key
    switch), TRGSW2NTT and launch gaps being the rest; then the ratio of the two forms' rates;
  - the latency of the 8 circuit bootstraps of one 8-bit address (the ROM read's selectors);
  - one 8-bit-address ROM read of a 256-entry ROM through the recorded per-gate API (address bits from the host, 8 circuit bootstraps,
    255 gCMUXNTT, the root fetched), ROM resident on the device, median of the repetitions; and the same read with the selectors
    circuit-bootstrapped on the host (the "without this feature" baseline: stage 1 by the CPU oracle's pieces on 16 threads, the
    private key switch in numpy, TRGSW2NTT of the host words into the holders, then the same CMUX tree).
The private key-switching key is random words: timing does not depend on them.  Usage: python tools/cb_times.py [reps]"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cufhe_amd as eng  # noqa: E402
import cb_checker as cb  # noqa: E402
import oracle_lib as ol  # noqa: E402

api = eng.api


def rom_read(st, rom, sels, make_selectors):
    """make_selectors(st) fills the 8 TrgswNtt holders `sels`; then the 255-CMUX tree over `rom`; returns ms to the fetched root"""
    eng.Synchronize()
    t0 = time.perf_counter()
    make_selectors(st)
    level = rom
    keep = []
    for k in range(8):
        nxt = []
        for j in range(len(level) // 2):
            o = api.Trlwe()
            api.gCMUXNTT(o, sels[k], level[2 * j + 1], level[2 * j], st)
            nxt.append(o)
        keep.append(nxt)
        level = nxt
    api.CtxtCopyD2H(level[0], st)
    eng.Synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = ol.load()
    keys = ol.Keys(L, seed=1)
    keys2 = ol.KeysLvl2(L, keys, seed=7)
    eng.SetGPUNum(1)
    eng.Initialize(keys.bk, keys.ksk)
    api.lvl2_initialize(keys2.bk, keys2.ksk)
    pksk = np.random.default_rng(1).integers(0, 2**32, size=cb.PKS_KEY_WORDS, dtype=np.uint32)
    api.cb_initialize(pksk)
    rng = np.random.default_rng(3)
    print("| inputs | rotations per input | ms / batch | CB/s | rotations ms | private KS ms | rest (TRGSW2NTT, gaps) ms | private KS share |")
    print("|---:|---:|---:|---:|---:|---:|---:|---:|")
    ratios = []
    for count in (1, 8, 64, 512, 4096):
        tl = keys.encrypt(rng.integers(0, 2, size=count).astype(np.uint8), 0, seed=count)
        d0 = api.DeviceBuffer(tl.size).upload(tl)
        dn = api.DeviceBuffer(count * cb.TRGSW_WORDS * 2)
        forms = (3, 1)
        for f in forms:                     # warm both forms (the half-wave key layout, the library's test-vector row)
            api.set_option("cb_rotations", f)
            api.circuit_bootstrap_batch(d0, count, trgsw_ntt=dn)
        eng.Synchronize()
        wall, br, ks = {f: [] for f in forms}, {f: [] for f in forms}, {f: [] for f in forms}
        for _ in range(reps):
            for f in forms:                 # alternated: both forms see the same clocks and the same neighbours
                api.set_option("cb_rotations", f)
                api.profile_enable(True)
                api.profile_get(reset=True)
                t0 = time.perf_counter()
                api.circuit_bootstrap_batch(d0, count, trgsw_ntt=dn)
                eng.Synchronize()
                wall[f].append((time.perf_counter() - t0) * 1e3)
                p = api.profile_get(reset=True)
                api.profile_enable(False)
                br[f].append(p.blind_rotate_ms)
                ks[f].append(p.keyswitch_ms)
        api.set_option("cb_rotations", 3)
        med = {}
        for f in forms:
            w, b, k = statistics.median(wall[f]), statistics.median(br[f]), statistics.median(ks[f])
            med[f] = w
            print(f"| {count} | {f} | {w:.3f} | {count / w * 1e3:.0f} | {b:.3f} | {k:.3f} | {w - b - k:.3f} | {100 * k / w:.1f} % |")
        ratios.append((count, med[3] / med[1]))
        del d0, dn
    print()
    print("one rotation against three, CB/s ratio: " + ", ".join(f"{c} inputs {r:.2f}x" for c, r in ratios))

    # the selectors of one 8-bit address
    tl = keys.encrypt(rng.integers(0, 2, size=8).astype(np.uint8), 0, seed=99)
    d0 = api.DeviceBuffer(tl.size).upload(tl)
    sel = api.DeviceBuffer(8 * cb.TRGSW_WORDS * 2)
    lat = []
    for _ in range(reps + 1):
        eng.Synchronize()
        t0 = time.perf_counter()
        api.circuit_bootstrap_batch(d0, 8, trgsw_ntt=sel)
        eng.Synchronize()
        lat.append((time.perf_counter() - t0) * 1e3)
    cb_ms = statistics.median(lat[1:])
    # host-side baseline: one selector's stage 1 by the oracle pieces (3 rotations) + stage 2 in numpy is far slower than any GPU
    # figure; measured on one selector here, x 8 for the address
    t0 = time.perf_counter()
    s1 = cb.cb_rotate_batch(keys2, tl[:1], threads=3)
    t_rot = time.perf_counter() - t0
    print()
    print(f"8 circuit bootstraps (one 8-bit address) on the GPU: {cb_ms:.3f} ms")
    print(f"host-side stage 1 of ONE circuit bootstrap (oracle pieces, 3 threads): {t_rot * 1e3:.0f} ms -> x 8 = {8 * t_rot * 1e3:.0f} ms "
          f"before the private key switch and the upload")
    del s1

    # one ROM read: device-side circuit bootstrapping against host-side
    st = api.Stream()
    rom = []
    for r in range(256):
        t = api.Trlwe()
        t.trlwehost[:] = rng.integers(0, 2**32, size=t.trlwehost.size, dtype=np.uint64).astype(np.uint32)
        api.CtxtCopyH2D(t, st)
        rom.append(t)
    bits = [api.Ctxt(0) for _ in range(8)]
    for k in range(8):
        bits[k].tlwehost[:] = tl[k]
    sels = [api.TrgswNtt() for _ in range(8)]

    def device_cb(s):
        for k in range(8):
            api.CircuitBootstrapping(sels[k], bits[k], s)

    def host_cb(s):
        st1 = cb.cb_rotate_batch(keys2, tl, threads=16)
        trgsw = cb.trgsw_from_stage1(pksk, st1)
        for k in range(8):
            eng.check(eng.lib.cufhe_amd_trgsw_to_ntt(s.device_id(), s.st(), trgsw[k].ctypes.data, sels[k]._h))

    dev = [rom_read(st, rom, sels, device_cb) for _ in range(reps + 1)][1:]
    host = rom_read(st, rom, sels, host_cb)
    print(f"one 8-bit-address ROM read (256 entries), recorded: {statistics.median(dev):.2f} ms (min {min(dev):.2f}); "
          f"with host-side circuit bootstrapping: {host:.0f} ms")


if __name__ == "__main__":
    main()
