"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle, word for word.

Mirrors the reference's own checks -- NTT product vs schoolbook
(test/test_polynomial_mult_1024.cu:209-223) and decrypt vs truth table for every gate
(test/test_gate_gpu.cc:72-84, test/test_util.h:75-94) -- and adds the stronger check the
exact arithmetic allows: identical ciphertext words.  Bit-exact, no tolerance.
"""
import os

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["batch", "half", "ll", "ll2"])
def br_kernel(request, engine):
    """Run a test once per blind-rotate kernel: wave-per-rotation (batch: two rotations per SIMD; half: one
    per SIMD, the tail shape), the 16-wave split-transform kernel (ll, lowest latency: a workgroup per rotation) and
    its two-rotations-per-workgroup form (ll2).  All must give the oracle's words."""
    which = request.param
    engine.api.set_option("ll2_threshold", 1 << 30 if which == "ll2" else 0)
    engine.api.set_option("ll_threshold", 1 << 30 if which == "ll" else 0)
    engine.api.set_option("half_threshold", 1 << 30 if which == "half" else 0)   # "batch": two rotations per SIMD whatever the count
    engine.api.set_option("ks_wg_threshold", 0 if which in ("batch", "half") else 1 << 30)
    engine.api.set_option("ks_split_threshold", 1 << 30 if which == "ll" else 0)   # ll: 8 workgroups per key switch
    yield which
    engine.api.set_option("ll2_threshold", -1)
    engine.api.set_option("ll_threshold", -1)
    engine.api.set_option("ks_wg_threshold", -1)
    engine.api.set_option("ks_split_threshold", -1)
    engine.api.set_option("half_threshold", -1)


def _upload(eng, arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    return eng.api.DeviceBuffer(arr.size).upload(arr)


def test_polymul_matches_schoolbook_and_oracle_ntt(engine, oracle):
    rng = np.random.default_rng(7)
    count = 64
    a = rng.integers(-32, 32, size=(count, ol.N), dtype=np.int32)
    a[0] = 31; a[1] = -32                      # extreme digits
    a[2] = rng.integers(-128, 129, size=ol.N)  # edge of the exactness bound
    b = rng.integers(0, 2**32, size=(count, ol.N), dtype=np.uint64).astype(np.uint32)
    b[0] = 0xFFFFFFFF; b[1] = 0x80000000; b[3] = 0
    da, db = _upload(engine, a.view(np.uint32)), _upload(engine, b)
    dres = engine.api.DeviceBuffer(count * ol.N)
    engine.polymul_batch(da, db, dres, count)
    got = dres.download().reshape(count, ol.N)
    for g in range(count):
        want = np.zeros(ol.N, np.uint32)
        oracle.orc_polymul_schoolbook(want, np.ascontiguousarray(a[g]), np.ascontiguousarray(b[g]))
        assert np.array_equal(got[g], want), f"product {g} differs from schoolbook"
        want2 = np.zeros(ol.N, np.uint32)
        oracle.orc_polymul_ntt(want2, np.ascontiguousarray(a[g]), np.ascontiguousarray(b[g]))
        assert np.array_equal(want, want2)


def test_polymul512_matches_schoolbook(engine):
    """The stand-alone 512-point transform (the wave code behind the low-latency kernel's half
    transforms) against a schoolbook negacyclic product mod (X^512 + 1, 2^32)."""
    rng = np.random.default_rng(8)
    count, n = 40, 512
    a = rng.integers(-128, 129, size=(count, n), dtype=np.int32)
    a[0] = 128; a[1] = -128
    b = rng.integers(0, 2**32, size=(count, n), dtype=np.uint64).astype(np.uint32)
    b[0] = 0x80000000; b[1] = 0x7FFFFFFF; b[2] = 0
    da, db = _upload(engine, a.view(np.uint32)), _upload(engine, b)
    dres = engine.api.DeviceBuffer(count * n)
    engine.polymul512_batch(da, db, dres, count)
    got = dres.download().reshape(count, n)
    for g in range(count):
        full = np.convolve(a[g].astype(np.int64), b[g].astype(np.int32).astype(np.int64))   # |sum| < 2^48: exact
        full = np.concatenate([full, np.zeros(2 * n - full.size, np.int64)])
        want = ((full[:n] - full[n:]) & 0xFFFFFFFF).astype(np.uint32)
        assert np.array_equal(got[g], want), f"product {g}"


@pytest.mark.parametrize("steps", [0, 1, 2, 3, 64, 65, 630])
def test_blind_rotate_accumulator_words(engine, keys, oracle, steps, br_kernel):
    count = 6 if steps == 630 else 10
    rng = np.random.default_rng(100 + steps)
    tl = rng.integers(0, 2**32, size=(count, ol.n + 1), dtype=np.uint64).astype(np.uint32)
    tl[0, :4] = 0                                  # abar = 0 steps
    tl[1, ol.n] = 0                                # bbar = 2N
    tl[2, ol.n] = 0xFFFFFFFF                       # bbar = 1
    tl[3, :8] = 0x7FFFFFFF
    tl[3, ol.n] = 0x80000000                       # bbar = N
    dt = _upload(engine, tl)
    dacc = engine.api.DeviceBuffer(count * 2 * ol.N)
    engine.blind_rotate_batch(dt, dacc, count, steps)
    got = dacc.download().reshape(count, 2 * ol.N)
    for g in range(count):
        want = np.zeros(2 * ol.N, np.uint32)
        oracle.orc_blind_rotate(keys.ek, want, np.ascontiguousarray(tl[g]), steps)
        assert np.array_equal(got[g], want), f"accumulator of rotation {g} differs after {steps} steps"


def test_blind_rotate_with_extreme_key_words(engine, keys, oracle, br_kernel):
    """Key words of maximal magnitude (0x80000000 = -2^31 in the signed reading, 0x7FFFFFFF, 0,
    0xFFFFFFFF): the sums then run closest to the p/2 exactness bound and the lazy residues
    closest to their limits."""
    rng = np.random.default_rng(17)
    ext = np.array([0x80000000, 0x7FFFFFFF, 0, 0xFFFFFFFF, 0x80000001], np.uint32)
    bk = ext[rng.integers(0, ext.size, ol.BK_WORDS)]
    bk[: 2 * 6 * 2 * ol.N] = 0x80000000          # steps 0 and 1: every word -2^31
    ek = oracle.orc_evalkey_create(bk, keys.ksk)
    engine.Initialize(bk, keys.ksk)
    try:
        count, steps = 6, 12
        tl = rng.integers(0, 2**32, size=(count, ol.n + 1), dtype=np.uint64).astype(np.uint32)
        dt = _upload(engine, tl)
        dacc = engine.api.DeviceBuffer(count * 2 * ol.N)
        engine.blind_rotate_batch(dt, dacc, count, steps)
        got = dacc.download().reshape(count, 2 * ol.N)
        for g in range(count):
            want = np.zeros(2 * ol.N, np.uint32)
            oracle.orc_blind_rotate(ek, want, np.ascontiguousarray(tl[g]), steps)
            assert np.array_equal(got[g], want), f"rotation {g} differs"
    finally:
        oracle.orc_evalkey_destroy(ek)
        engine.Initialize(keys.bk, keys.ksk)


def test_keyswitch_words(engine, keys, oracle, br_kernel):
    count = 16
    rng = np.random.default_rng(5)
    t1 = rng.integers(0, 2**32, size=(count, ol.N + 1), dtype=np.uint64).astype(np.uint32)
    t1[0] = 0
    t1[1] = 0xFFFFFFFF
    d1 = _upload(engine, t1)
    d0 = engine.api.DeviceBuffer(count * (ol.n + 1))
    engine.keyswitch_batch(d1, d0, count)
    got = d0.download().reshape(count, ol.n + 1)
    for g in range(count):
        want = np.zeros(ol.n + 1, np.uint32)
        oracle.orc_keyswitch(keys.ek, want, np.ascontiguousarray(t1[g]))
        assert np.array_equal(got[g], want)


@pytest.mark.parametrize("count", [1, 2, 3, 33, 257, 1031])
def test_keyswitch_shared_table_groupings(engine, keys, oracle, count):
    """The shared-table key switch (the ciphertexts of a workgroup share each step of the key through LDS, a wave per ciphertext):
    odd counts, a last workgroup that is not full, the largest and the smallest number of ciphertexts per workgroup -- every word
    equal to the workgroup-per-ciphertext kernel's, first and last ciphertext equal to the oracle's.  The eight-workgroup form of the
    direct kernel (the default of small launches) gives the same words at every count."""
    rng = np.random.default_rng(4100 + count)
    t1 = rng.integers(0, 2**32, size=(count, ol.N + 1), dtype=np.uint64).astype(np.uint32)
    t1[0, : ol.N] = 0xFFFFFFFF
    d1 = _upload(engine, t1)
    d0 = engine.api.DeviceBuffer(count * (ol.n + 1))

    def run(split, wg, per, slices=-1):
        engine.api.set_option("ks_split_threshold", split)
        engine.api.set_option("ks_wg_threshold", wg)
        engine.api.set_option("ks_per_wg", per)
        engine.api.set_option("ks_slices", slices)
        try:
            d0.upload(np.full(count * (ol.n + 1), 0xDEADBEEF, np.uint32))
            engine.keyswitch_batch(d1, d0, count)
            return d0.download().reshape(count, ol.n + 1).copy()
        finally:
            for k in ("ks_split_threshold", "ks_wg_threshold", "ks_per_wg", "ks_slices"):
                engine.api.set_option(k, -1)

    ref = run(0, 1 << 30, -1)                      # one workgroup per ciphertext
    for g in (0, count - 1):
        want = np.zeros(ol.n + 1, np.uint32)
        oracle.orc_keyswitch(keys.ek, want, np.ascontiguousarray(t1[g]))
        assert np.array_equal(ref[g], want)
    assert np.array_equal(run(1 << 30, 0, -1), ref), f"eight workgroups per ciphertext, {count} ciphertexts"
    # (ciphertexts per workgroup, runs the steps of j are cut into: above one the partial sums meet in the output through atomics)
    for per, slices in ((-1, -1), (1, 1), (6, 1), (16, 1), (16, 2), (9, 4), (-1, 16), (16, 64)):
        got = run(0, 0, per, slices)
        assert np.array_equal(got, ref), f"shared-table key switch, {count} ciphertexts, {per} per workgroup, {slices} runs of j"


@pytest.mark.parametrize("level", [0, 1])
def test_every_gate_words_and_truth_table(engine, keys, oracle, level, br_kernel):
    """All 14 ops on all input combinations: words == oracle, decrypt == truth table."""
    combos = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)], np.uint8)
    count = len(combos)
    ins = [keys.encrypt(combos[:, i], level, seed=900 + 10 * level + i) for i in range(3)]
    dins = [_upload(engine, x) for x in ins]
    dout = engine.api.DeviceBuffer(count * ol.LVL_WORDS[level])
    for op in range(14):
        engine.gate_batch(op, level, dout, dins[0], dins[1], dins[2], count=count)
        got = dout.download().reshape(count, -1)
        want = keys.gate_batch(op, level, ins[0], ins[1], ins[2])
        assert np.array_equal(got, want), f"{ol.OPS[op]} level {level}: ciphertext words differ from the oracle"
        bits = keys.decrypt(got, level)
        exp = [ol.truth(oracle, op, *c) for c in combos]
        assert list(bits) == exp, f"{ol.OPS[op]} level {level}: decrypt != truth table"


def test_mixed_batch_and_aliasing(engine, keys, oracle, br_kernel):
    """Mixed op codes in one launch (BASELINE config 3 shape) with out aliasing in0."""
    count = 64
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 2, size=(3, count)).astype(np.uint8)
    ins = [keys.encrypt(bits[i], 0, seed=1200 + i) for i in range(3)]
    ops = np.array([[ol.OPS.index(x) for x in ("AND", "OR", "XOR", "NAND", "MUX", "NOT", "COPY", "NMUX")][g % 8]
                    for g in range(count)], np.int32)
    dins = [_upload(engine, x) for x in ins]
    engine.gate_batch(ops, 0, dins[0], dins[0], dins[1], dins[2], count=count)   # out == in0
    got = dins[0].download().reshape(count, -1)
    want = keys.gate_batch(ops, 0, ins[0], ins[1], ins[2])
    assert np.array_equal(got, want)
    exp = [ol.truth(oracle, int(ops[g]), bits[0, g], bits[1, g], bits[2, g]) for g in range(count)]
    assert list(keys.decrypt(got, 0)) == exp


def test_reference_api_mirror_streams(engine, keys, oracle):
    """The per-gate Stream/Ctxt surface (test/test_gate_gpu.cc, test/test_api_gpu.cu:140-159):
    chained gates on one stream with out aliasing an input, completion via Synchronize."""
    api = engine.api
    nst, per = 4, 3
    sts = [api.Stream() for _ in range(nst)]
    for s in sts:
        s.Create()
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2, size=(2, nst * per)).astype(np.uint8)
    cts = [[api.Ctxt(0) for _ in range(nst * per)] for _ in range(2)]
    enc = [keys.encrypt(bits[i], 0, seed=77 + i) for i in range(2)]
    for i in range(2):
        for g in range(nst * per):
            cts[i][g].tlwehost[:] = enc[i][g]
    for g in range(nst * per):
        st = sts[g % nst]
        api.Nand(cts[0][g], cts[0][g], cts[1][g], st)     # ct = Nand(ct, b)
        api.Or(cts[0][g], cts[0][g], cts[1][g], st)       # ct = Or(ct, b)
    api.Synchronize()
    assert all(api.StreamQuery(s) for s in sts)
    assert all(c.tlwedevices[0] for c in cts[0])          # tlwedevices: one device buffer per GPU
    for g in range(nst * per):
        a, b = int(bits[0, g]), int(bits[1, g])
        exp = (1 - a * b) | b
        assert keys.decrypt(cts[0][g].tlwehost, 0)[0] == exp
    for s in sts:
        s.Destroy()


def test_batch_4096_nand_decrypts(engine, keys):
    """BASELINE config 2 at full size: every output decrypts to NAND; a sampled subset is
    compared word for word with the oracle."""
    count = 4096
    rng = np.random.default_rng(42)
    bits = rng.integers(0, 2, size=(2, count)).astype(np.uint8)
    ins = [keys.encrypt(bits[i], 0, seed=4200 + i) for i in range(2)]
    dins = [_upload(engine, x) for x in ins]
    dout = engine.api.DeviceBuffer(count * (ol.n + 1))
    engine.gate_batch(ol.OPS.index("NAND"), 0, dout, dins[0], dins[1], count=count)
    got = dout.download().reshape(count, -1)
    assert np.array_equal(keys.decrypt(got, 0), 1 - bits[0] * bits[1])
    idx = np.arange(0, count, 64)
    want = keys.gate_batch(ol.OPS.index("NAND"), 0, ins[0][idx], ins[1][idx])
    assert np.array_equal(got[idx], want)


def test_golden_vectors_on_gpu(engine, keys):
    """tests/golden/golden_v1.json: every op, both levels, sha256 of the output words."""
    import hashlib
    import json
    import os
    with open(os.path.join(ol.ROOT, "tests", "golden", "golden_v1.json")) as f:
        g = json.load(f)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint32).tobytes()).hexdigest()
    # a fixture that cannot be reproduced is a failure, not a skip: the keys are regenerated from the
    # committed seed by integer arithmetic and a Box-Muller in double precision (oracle/tfhe_oracle.c)
    assert sha(keys.bk) == g["keys_sha256"]["bk"] and sha(keys.ksk) == g["keys_sha256"]["ksk"], \
        "seeded key generation no longer reproduces tests/golden/golden_v1.json (keys_sha256)"
    triples = np.array(g["triples"], np.uint8)
    for level in (0, 1):
        ins = [keys.encrypt(triples[:, i], level, seed=5000 + 100 * level + i) for i in range(3)]
        assert [sha(x) for x in ins] == g["levels"][str(level)]["inputs_sha256"]
        dins = [_upload(engine, x) for x in ins]
        dout = engine.api.DeviceBuffer(len(triples) * ol.LVL_WORDS[level])
        for op, name in enumerate(ol.OPS):
            engine.gate_batch(op, level, dout, dins[0], dins[1], dins[2], count=len(triples))
            got = dout.download().reshape(len(triples), -1)
            assert sha(got) == g["levels"][str(level)]["ops"][name]["out_sha256"], (name, level)


def test_scheduler_hazards_and_g_gates(engine, keys, oracle):
    """Dependences inside what would be one batch: RAW chains, WAR, shared inputs, g-gates
    with explicit copies, StreamQuery-driven completion."""
    api = engine.api
    st = api.Stream()
    st.Create()
    a, b, c, o1, o2 = (api.Ctxt(1) for _ in range(5))
    bits = dict(a=1, b=0, c=1)
    seeds = dict(a=611, b=612, c=613)      # fixed: hash(str) is randomised per process
    for ct, name in ((a, "a"), (b, "b"), (c, "c")):
        ct.tlwehost[:] = keys.encrypt([bits[name]], 1, seed=seeds[name])[0]
    api.And(o1, a, b, st)            # o1 = a & b = 0
    api.Or(o2, o1, c, st)            # RAW on o1: o2 = 0 | 1 = 1
    api.Xor(a, a, c, st)             # WAR/RAW on a: a = 1 ^ 1 = 0   (And above must have read the old a)
    api.Nand(o1, o2, a, st)          # WAW on o1: o1 = !(1 & 0) = 1
    while not api.StreamQuery(st):
        pass
    assert [int(keys.decrypt(x.tlwehost, 1)[0]) for x in (o1, o2, a)] == [1, 1, 0]
    # device-resident chain with explicit copies
    api.CtxtCopyH2D(b, st); api.CtxtCopyH2D(c, st)
    api.gOr(o1, b, c, st)            # 0 | 1 = 1
    api.gAndNY(o2, o1, c, st)        # !1 & 1 = 0
    api.CtxtCopyD2H(o2, st); api.CtxtCopyD2H(o1, st)
    api.Synchronize()
    assert [int(keys.decrypt(x.tlwehost, 1)[0]) for x in (o1, o2)] == [1, 0]
    st.Destroy()


def _variant_env(**extra):
    """The variants of the C++ program (more logical GPUs, renaming off) repeat what test_cpp_gate_api_mirror ran in full; by default they
    skip its three at-size parts (4096 bootstraps + Refresh, 32768 mixed gates, the N = 2048 ring), which do not depend on the variant:
    the suite stays well inside the driver's time limit on a slow box.  CUFHE_AMD_FULL_GPU_SUITE=1 runs everything everywhere."""
    import os
    env = dict(os.environ, **extra)
    if not os.environ.get("CUFHE_AMD_FULL_GPU_SUITE"):
        env["CUFHE_AMD_TEST_SKIP_AT_SIZE"] = "1"
    return env


def test_cpp_gate_api_mirror(engine):
    """tests/cpp/test_gate_api.cpp: the reference's own test programs (test_gate_gpu.cc,
    test_gate_gpu_multi.cc, test_intensive.cc, test_api_gpu.cu) against include/cufhe_amd.hpp,
    compiled with plain g++ (host code stays C++)."""
    import os
    import subprocess
    import cpp_build
    exe = cpp_build.build_gate_api("test_gate_api")
    engine.CleanUp()                      # the C++ program owns the device state while it runs
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        import oracle_lib
        k = oracle_lib.Keys(oracle_lib.load(), seed=1)
        engine.SetGPUNum(1)
        engine.Initialize(k.bk, k.ksk)


def test_cpp_gate_api_tfhepp_branch(engine):
    """The same source compiled with -DCUFHE_AMD_USE_TFHEPP over tests/cpp/tfhepp_stub (tests/test_capi.py builds it on the CPU):
    keys handed over as a TFHEpp::EvalKey (Initialize(ek), lvl2::Initialize(ek)), every gate of both levels decrypt-checked."""
    import os
    import subprocess
    import cpp_build
    exe = cpp_build.build_gate_api("test_gate_api_tfhepp", tfhepp=True)
    engine.CleanUp()
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, CUFHE_AMD_TEST_QUICK="1"))
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        import oracle_lib
        k = oracle_lib.Keys(oracle_lib.load(), seed=1)
        engine.SetGPUNum(1)
        engine.Initialize(k.bk, k.ksk)


@pytest.mark.parametrize("name", ["cggi16", "k2n512", "smallmod", "cggi16-tfhepp", "k2n512-tfhepp"])
def test_cpp_gate_api_on_a_parameter_set(engine, name):
    """The reference's own test programs (tests/cpp/test_gate_api.cpp: test_gate_gpu.cc on lvl1 ciphertexts, test_gate_gpu_multi.cc on
    lvl0, test_api_gpu.cu's chains, test_intensive.cc, the ripple-carry adders, test_perf.cc's bootstraps to a TRLWE and -- except on
    the small-modulus build, as in the reference -- test_cmux.cc's CMUXNTT / TRGSW2NTT) on another parameter set, chosen the way the
    reference chooses: ONE selector, the numbers of the parameter structs (CMakeLists.txt:8-24, include/bootstrap_gpu.cuh:51-53).
    include/cufhe_amd.hpp finds the library's set from those numbers.  `<set>`: the stand-in structs of the header take the set's
    numbers (-DCUFHE_AMD_PARAM_SET_<SET>; `smallmod` with the reference's own -DUSE_SMALL_NTT_MODULUS, CMakeLists.txt:26-28);
    `<set>-tfhepp`: -DCUFHE_AMD_USE_TFHEPP over tests/cpp/tfhepp_stub built with TFHEpp's own macro (USE_80BIT_SECURITY / USE_CONCRETE)
    and NOTHING naming a set of this library.  -DORC_SET_<SET> selects the oracle's key generation and decryption."""
    import os
    import subprocess
    import cpp_build
    base = name.split("-")[0]
    if name.endswith("-tfhepp"):
        defines = ["-DUSE_80BIT_SECURITY" if base == "cggi16" else "-DUSE_CONCRETE", "-DORC_SET_" + base.upper()]
    else:
        defines = ["-DUSE_SMALL_NTT_MODULUS" if base == "smallmod" else "-DCUFHE_AMD_PARAM_SET_" + base.upper(), "-DORC_SET_" + base.upper()]
    exe = cpp_build.build_gate_api("test_gate_api_" + name.replace("-", "_"), defines=defines, oracle="oracle_" + base, tfhepp=name.endswith("-tfhepp"))
    engine.CleanUp()
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        import oracle_lib
        k = oracle_lib.Keys(oracle_lib.load(), seed=1)
        engine.SetGPUNum(1)
        engine.Initialize(k.bk, k.ksk)


def test_cpp_gate_api_three_logical_gpus(engine):
    """The same program with SetGPUNum(3) (test/test_gate_gpu_multi.cc:36-93: default-constructed streams
    round-robin the devices, include/cufhe_gpu.cuh:154-159): per-device key replicas, schedulers, launch threads
    and ciphertext buffers.  The box has one GPU, so the three logical devices share it ("share_devices")."""
    import os
    import subprocess
    exe = os.path.join(ol.ROOT, "tests", "cpp", "test_gate_api")
    assert os.path.exists(exe), "built by test_cpp_gate_api_mirror"
    engine.CleanUp()
    try:
        out = subprocess.run([exe, "3"], capture_output=True, text=True, timeout=900, env=_variant_env(CUFHE_AMD_SHARE_DEVICES="1"))
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        import oracle_lib
        k = oracle_lib.Keys(oracle_lib.load(), seed=1)
        engine.SetGPUNum(1)
        engine.Initialize(k.bk, k.ksk)


def test_cpp_gate_api_without_output_renaming(engine):
    """The same program, two logical devices, with "sched_rename" 0 (the default is 1: every other run of this
    program renames): every check of the reference's test programs (truth tables, chained in-place gates, polling,
    device-resident g-gates, TRLWE-level primitives, launch-count bounds, tlwedevices after Synchronize) holds when every
    output waits for the users of its buffer instead."""
    import os
    import subprocess
    exe = os.path.join(ol.ROOT, "tests", "cpp", "test_gate_api")
    assert os.path.exists(exe), "built by test_cpp_gate_api_mirror"
    engine.CleanUp()
    try:
        out = subprocess.run([exe, "2"], capture_output=True, text=True, timeout=900,
                             env=_variant_env(CUFHE_AMD_SHARE_DEVICES="1", CUFHE_AMD_NO_SCHED_RENAME="1"))
        print(out.stdout[-3000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        import oracle_lib
        k = oracle_lib.Keys(oracle_lib.load(), seed=1)
        engine.SetGPUNum(1)
        engine.Initialize(k.bk, k.ksk)


def test_plain_bootstrap(engine, keys, oracle, br_kernel):
    """Bootstrap (src/bootstrap_gpu.cu:290-301): blind rotate -> extract -> key switch of one TLWE."""
    rng = np.random.default_rng(31)
    bits = rng.integers(0, 2, 12).astype(np.uint8)
    cts = keys.encrypt(bits, 0, seed=909)
    din = _upload(engine, cts)
    dout = engine.api.DeviceBuffer(cts.size)
    engine.bootstrap_batch(dout, din, len(bits))
    got = dout.download().reshape(len(bits), -1)
    for g in range(len(bits)):
        acc = np.zeros(2 * ol.N, np.uint32)
        oracle.orc_blind_rotate(keys.ek, acc, np.ascontiguousarray(cts[g]), -1)
        t1 = np.zeros(ol.N + 1, np.uint32)
        oracle.orc_sample_extract0(t1, acc)
        t0 = np.zeros(ol.n + 1, np.uint32)
        oracle.orc_keyswitch(keys.ek, t0, t1)
        assert np.array_equal(got[g], t0)
    assert np.array_equal(keys.decrypt(got, 0), bits)


def test_keys_and_ciphertexts_through_cereal_files(engine, keys, tmp_path):
    """SURVEY.md 8 f3 on the GPU path: the evaluation key goes through include/cufhe_amd_cereal.hpp (SaveEvalKey -> file ->
    LoadEvalKey, header size found by the reader) into cufhe::Initialize, the inputs through a std::vector<TLWE<lvl0param>>
    archive, 24 cufhe::Nand gates run, and the output archive == the oracle's words.  (The file code stays UNVERIFIED
    against TFHEpp-produced files -- none exists here; this only keeps it on a path that reaches the device.)"""
    import struct
    import subprocess
    src = os.path.join(ol.ROOT, "tests", "cpp", "test_cereal_keys.cpp")
    exe = os.path.join(ol.ROOT, "tests", "cpp", "test_cereal_keys")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src, "-L" + os.path.join(ol.ROOT, "cufhe_amd"), "-lcufhe_amd",
                           "-Wl,-rpath," + os.path.join(ol.ROOT, "cufhe_amd")])
    count = 24
    bits = np.random.default_rng(77).integers(0, 2, size=(2, count)).astype(np.uint8)
    ins = [keys.encrypt(bits[i], 0, seed=770 + i) for i in range(2)]
    (tmp_path / "bk.raw").write_bytes(np.ascontiguousarray(keys.bk, np.uint32).tobytes())
    (tmp_path / "ksk.raw").write_bytes(np.ascontiguousarray(keys.ksk, np.uint32).tobytes())
    for i in range(2):      # cereal portable binary: endianness flag, size tag, the arrays back to back
        (tmp_path / f"in{i}.bin").write_bytes(b"\x01" + struct.pack("<Q", count) + np.ascontiguousarray(ins[i], np.uint32).tobytes())
    engine.CleanUp()                      # the C++ program owns the device state while it runs
    try:
        out = subprocess.run([exe, tmp_path / "bk.raw", tmp_path / "ksk.raw", tmp_path / "in0.bin", tmp_path / "in1.bin",
                              tmp_path / "out.bin", tmp_path / "ek.bin"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and f"ok {count}" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
        assert "header 53 members 4 bk_member 1 ksk_member 3" in out.stdout, out.stdout
    finally:
        engine.SetGPUNum(1)
        engine.Initialize(keys.bk, keys.ksk)
    blob = (tmp_path / "out.bin").read_bytes()
    assert blob[0] == 1 and struct.unpack("<Q", blob[1:9])[0] == count
    got = np.frombuffer(blob[9:], np.uint32).reshape(count, ol.n + 1)
    assert np.array_equal(got, keys.gate_batch(0, 0, ins[0], ins[1]))
    assert list(keys.decrypt(got, 0)) == list(1 - bits[0] * bits[1])


def test_cpp_legacy_manual_program(engine):
    """tests/cpp/test_legacy_api.cpp: the reference's user-manual program (README.md:46-82,
    test/test_api_gpu.cu) -- KeyGen, Encrypt, Initialize(pub_key), nine chained in-place gates on
    32 streams, Decrypt -- against include/cufhe_amd_legacy.hpp."""
    import os
    import subprocess
    src = os.path.join(ol.ROOT, "tests", "cpp", "test_legacy_api.cpp")
    exe = os.path.join(ol.ROOT, "tests", "cpp", "test_legacy_api")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, src,
                           "-L" + os.path.join(ol.ROOT, "cufhe_amd"), "-lcufhe_amd",
                           "-Wl,-rpath," + os.path.join(ol.ROOT, "cufhe_amd")])
    engine.CleanUp()
    try:
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        print(out.stdout[-2000:])
        assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    finally:
        import oracle_lib
        k = oracle_lib.Keys(oracle_lib.load(), seed=1)
        engine.SetGPUNum(1)
        engine.Initialize(k.bk, k.ksk)


def test_trlwe_level_primitives(engine, keys, oracle):
    """SampleExtractAndKeySwitch, Refresh, TRGSW2NTT + CMUXNTT (src/cufhe_gates_gpu.cu:69-146):
    words identical to the oracle; Refresh keeps the plaintext (test/test_perf.cc:83-87)."""
    count = 6
    rng = np.random.default_rng(21)
    # TRLWEs produced by real blind rotations of encryptions of known bits
    bits = np.array([0, 1, 1, 0, 1, 0], np.uint8)
    cts = keys.encrypt(bits, 0, seed=333)
    trl = np.zeros((count, 2 * ol.N), np.uint32)
    for g in range(count):
        oracle.orc_blind_rotate(keys.ek, trl[g], np.ascontiguousarray(cts[g]), -1)
    dtrl = _upload(engine, trl)
    # SEI + KS
    d0 = engine.api.DeviceBuffer(count * (ol.n + 1))
    engine.api.sample_extract_keyswitch_batch(dtrl, d0, count)
    got = d0.download().reshape(count, -1)
    for g in range(count):
        want = np.zeros(ol.n + 1, np.uint32)
        oracle.orc_sample_extract_keyswitch(keys.ek, want, np.ascontiguousarray(trl[g]))
        assert np.array_equal(got[g], want)
    assert list(keys.decrypt(got, 0)) == list(bits)
    # Refresh
    dout = engine.api.DeviceBuffer(count * 2 * ol.N)
    engine.api.refresh_batch(dtrl, dout, count)
    got = dout.download().reshape(count, -1)
    for g in range(count):
        want = np.zeros(2 * ol.N, np.uint32)
        oracle.orc_refresh(keys.ek, want, np.ascontiguousarray(trl[g]))
        assert np.array_equal(got[g], want)
        t1 = np.zeros(ol.N + 1, np.uint32)
        oracle.orc_sample_extract0(t1, np.ascontiguousarray(got[g]))
        assert keys.decrypt(t1, 1)[0] == bits[g]
    # CMUX with random TRGSW words (exactness does not depend on the key being valid)
    trgsw = rng.integers(0, 2**32, size=(count, 6, 2, ol.N), dtype=np.uint64).astype(np.uint32)
    c1 = rng.integers(0, 2**32, size=(count, 2 * ol.N), dtype=np.uint64).astype(np.uint32)
    c0 = rng.integers(0, 2**32, size=(count, 2 * ol.N), dtype=np.uint64).astype(np.uint32)
    c1[0] = c0[0]                                   # zero difference: res = c0
    dtg, dc1, dc0 = _upload(engine, trgsw), _upload(engine, c1), _upload(engine, c0)
    dntt = engine.api.DeviceBuffer(count * 12 * ol.N * 2)        # doubles = 2 words each
    engine.api.trgsw_to_ntt_batch(dtg, dntt, count)
    dres = engine.api.DeviceBuffer(count * 2 * ol.N)
    engine.api.cmux_batch(dntt, dc1, dc0, dres, count)
    got = dres.download().reshape(count, -1)
    assert np.array_equal(got[0], c0[0])
    for g in range(count):
        want = np.zeros(2 * ol.N, np.uint32)
        oracle.orc_cmux(want, np.ascontiguousarray(trgsw[g]).ravel(), np.ascontiguousarray(c1[g]), np.ascontiguousarray(c0[g]))
        assert np.array_equal(got[g], want)


def test_refresh_batch_in_place(engine, keys, oracle):
    """refresh_batch with trlwe_out == trlwe_in at 9 TRLWEs (one 8-rotation workgroup plus one): the rotations' results go through
    scratch and are copied over their own inputs, so every row must still be the oracle's sample extract -> key switch ->
    blind rotate of the row that was there before the call."""
    count = 9
    bits = np.array([1, 0, 0, 1, 1, 0, 1, 1, 0], np.uint8)
    cts = keys.encrypt(bits, 0, seed=334)
    trl = np.zeros((count, 2 * ol.N), np.uint32)
    for g in range(count):
        oracle.orc_blind_rotate(keys.ek, trl[g], np.ascontiguousarray(cts[g]), -1)
    dtrl = _upload(engine, trl)
    engine.api.refresh_batch(dtrl, dtrl, count)
    got = dtrl.download().reshape(count, -1)
    for g in range(count):
        t0 = np.zeros(ol.n + 1, np.uint32)
        oracle.orc_sample_extract_keyswitch(keys.ek, t0, np.ascontiguousarray(trl[g]))
        want = np.zeros(2 * ol.N, np.uint32)
        oracle.orc_blind_rotate(keys.ek, want, t0, -1)
        assert np.array_equal(got[g], want), g
        t1 = np.zeros(ol.N + 1, np.uint32)
        oracle.orc_sample_extract0(t1, np.ascontiguousarray(got[g]))
        assert keys.decrypt(t1, 1)[0] == bits[g]


@pytest.mark.parametrize("count", [1, 7, 9, 17, 129, 300, 1031])
def test_ragged_batch_sizes(engine, keys, count):
    """Batch sizes that are not multiples of the 8-rotation / 16-ciphertext workgroups, on both
    sides of the kernel-selection thresholds; every output must decrypt correctly and a
    sample is compared word for word with the oracle."""
    rng = np.random.default_rng(count)
    bits = rng.integers(0, 2, size=(2, count)).astype(np.uint8)
    ins = [keys.encrypt(bits[i], 0, seed=7000 + count + i) for i in range(2)]
    dins = [_upload(engine, x) for x in ins]
    dout = engine.api.DeviceBuffer(count * (ol.n + 1))
    for thr in (0, 1 << 30):            # batch kernels, then low-latency kernels
        if thr and count > 300:
            continue                     # one workgroup per rotation: keep the test short
        engine.api.set_option("ll_threshold", thr if thr else -1)
        engine.api.set_option("ks_wg_threshold", thr)
        try:
            dout.upload(np.zeros(count * (ol.n + 1), np.uint32))
            engine.gate_batch(ol.OPS.index("XOR"), 0, dout, dins[0], dins[1], count=count)
            got = dout.download().reshape(count, -1)
        finally:
            engine.api.set_option("ll_threshold", -1)
            engine.api.set_option("ks_wg_threshold", -1)
        assert np.array_equal(keys.decrypt(got, 0), bits[0] ^ bits[1])
        idx = np.unique(np.array([0, count // 2, count - 1]))
        want = keys.gate_batch(ol.OPS.index("XOR"), 0, ins[0][idx], ins[1][idx])
        assert np.array_equal(got[idx], want)


@pytest.mark.parametrize("count,opts", [(700, dict(ll_threshold=0, ll2_threshold=0)),        # one rotation per SIMD (4 of 8 waves)
                                        (1100, dict(ll2_threshold=0)), (3200, dict(ll2_threshold=0)),   # (rounds +) 1024 at one per SIMD + low-latency kernel
                                        (300, {}), (600, {}), (1300, {}), (1536, {}), (3500, {}),       # paired low-latency kernel: all / 512 + single kernel / tail
                                        (2049, {}), (2700, {}), (4600, {})])                  # full rounds + a tail
def test_launch_shapes_with_tails(engine, keys, count, opts):
    """Launches that do not fill whole rounds of the blind-rotate grid are cut into full rounds plus a
    tail on a cheaper kernel (launch_plan.h, plan_blind_rotate): every output must still decrypt, sampled
    outputs -- first, last, and both sides of every cut -- must be the oracle's words."""
    rng = np.random.default_rng(count)
    bits = rng.integers(0, 2, size=(2, count)).astype(np.uint8)
    ins = [keys.encrypt(bits[i], 0, seed=7700 + count + i) for i in range(2)]
    dins = [_upload(engine, x) for x in ins]
    dout = engine.api.DeviceBuffer(count * (ol.n + 1))
    for k, v in opts.items():
        engine.api.set_option(k, v)
    try:
        engine.gate_batch(ol.OPS.index("NAND"), 0, dout, dins[0], dins[1], count=count)
        got = dout.download().reshape(count, -1)
    finally:
        engine.api.set_option("ll_threshold", -1)
        engine.api.set_option("ll2_threshold", -1)
    assert np.array_equal(keys.decrypt(got, 0), 1 - bits[0] * bits[1])
    # the cuts are in units of the device's CU count (launch_plan.h: plan_blind_rotate): a grid round is 8 rotations per CU
    cus = engine.api.device_cus()
    cut = count - count % (8 * cus)
    idx = np.unique(np.clip(np.array([0, 3, 4, 7, cut - 1, cut, cut + 3, cut + 4, cut + 2 * cus - 1, cut + 2 * cus, cut + 2 * cus + 1, cut + 4 * cus - 1,
                                      cut + 4 * cus, cut + 4 * cus + 3, count - 5, count - 2, count - 1]), 0, count - 1))
    want = keys.gate_batch(ol.OPS.index("NAND"), 0, ins[0][idx], ins[1][idx])
    assert np.array_equal(got[idx], want)


@pytest.mark.parametrize("cus", [40, 104])
def test_launch_and_flush_rules_follow_the_cu_count(engine, keys, cus):
    """No rule is tied to MI355X's 256 CUs: with "cus_override" (a partitioned device, another chip) the blind rotation is cut at
    multiples of 8 x cus -- visible in the number of launches -- and the per-gate API flushes a full level at two such rounds; the
    words do not change."""
    api = engine.api
    api.set_option("cus_override", cus)
    try:
        assert api.device_cus() == cus
        count = 8 * cus + cus + 3                 # one full round + a tail of a little more than one rotation per CU
        rng = np.random.default_rng(cus)
        bits = rng.integers(0, 2, size=(2, count)).astype(np.uint8)
        ins = [keys.encrypt(bits[i], 0, seed=8800 + cus + i) for i in range(2)]
        dins = [_upload(engine, x) for x in ins]
        dout = api.DeviceBuffer(count * (ol.n + 1))
        api.profile_enable(True)
        api.profile_get(reset=True)
        engine.gate_batch(ol.OPS.index("XOR"), 0, dout, dins[0], dins[1], count=count)
        got = dout.download().reshape(count, -1)
        prof = api.profile_get(reset=True)
        api.profile_enable(False)
        assert prof.blind_rotations == count and prof.blind_rotate_launches == 1      # one launch SEQUENCE (rounds + tail inside it)
        assert np.array_equal(keys.decrypt(got, 0), bits[0] ^ bits[1])
        cut = 8 * cus
        idx = np.unique(np.clip(np.array([0, cut - 1, cut, cut + cus - 1, cut + cus, cut + 2 * cus - 1, cut + 2 * cus, count - 1]), 0, count - 1))
        assert np.array_equal(got[idx], keys.gate_batch(ol.OPS.index("XOR"), 0, ins[0][idx], ins[1][idx]))
        # the scheduler: on the idle device a level is launched at ONE grid round of this CU count, behind it at TWO
        rnd = 8 * cus
        n = 3 * rnd
        cts = [api.Ctxt(0) for _ in range(3 * n)]
        enc = keys.encrypt(rng.integers(0, 2, size=2 * n).astype(np.uint8), 0, seed=8900 + cus)
        for i in range(2 * n):
            cts[n + i].tlwehost[:] = enc[i]
        st = api.Stream()
        st.Create()
        api.Synchronize()
        api.sched_stats(reset=True)
        for i in range(rnd - 1):
            api.Nand(cts[i], cts[n + i], cts[2 * n + i], st)
        assert api.sched_stats().groups == 0
        api.Nand(cts[rnd - 1], cts[n + rnd - 1], cts[2 * n + rnd - 1], st)
        assert api.sched_stats().groups == 1, f"the idle device was not handed the first round of {rnd} gates"
        for i in range(rnd, n - 1):
            api.Nand(cts[i], cts[n + i], cts[2 * n + i], st)
        assert api.sched_stats().groups == 1
        api.Nand(cts[n - 1], cts[2 * n - 1], cts[3 * n - 1], st)
        assert api.sched_stats().groups == 2, f"a level of two rounds ({2 * rnd} gates) was not launched behind the running one"
        api.Synchronize()
        assert api.sched_stats().max_level_gates == 2 * rnd
        pick = np.array([0, rnd - 1, rnd, n - 1])
        want = keys.gate_batch(ol.OPS.index("NAND"), 0, enc[pick], enc[n + pick])
        assert np.array_equal(np.stack([cts[i].tlwehost for i in pick]), want)
        st.Destroy()
    finally:
        api.profile_enable(False)
        api.set_option("cus_override", 0)


def test_failed_initialize_keeps_the_loaded_keys(engine, keys, oracle):
    """Initialize(ek) builds the new keys beside the loaded ones and swaps at the end (capi.hip: cufhe_amd_initialize): when an
    allocation fails on the way -- every one of the call's three, through the "test_fail_alloc" hook -- the call reports -2, the OLD
    keys still produce their words, and no device memory is lost."""
    api = engine.api
    other = ol.Keys(oracle, seed=2)
    count = 5
    bits = np.array([[0, 1, 0, 1, 1], [0, 0, 1, 1, 0]], np.uint8)
    ins = [keys.encrypt(bits[i], 0, seed=3300 + i) for i in range(2)]
    d0, d1 = _upload(engine, ins[0]), _upload(engine, ins[1])
    dout = api.DeviceBuffer(count * (ol.n + 1))
    want_old = keys.gate_batch(ol.OPS.index("NAND"), 0, ins[0], ins[1]).reshape(count, -1)
    api.Synchronize()
    free0, _ = api.device_mem_info()
    try:
        for nth in range(3):
            api.set_option("test_fail_alloc", nth)
            with pytest.raises(engine.CufheAmdError):
                engine.Initialize(other.bk, other.ksk)
            engine.gate_batch(ol.OPS.index("NAND"), 0, dout, d0, d1, count=count)
            assert np.array_equal(dout.download().reshape(count, -1), want_old), f"allocation {nth} failed and took the loaded keys with it"
        api.Synchronize()
        free1, _ = api.device_mem_info()
        assert abs(free0 - free1) < (32 << 20), "failed Initialize calls leaked device memory"
        engine.Initialize(other.bk, other.ksk)            # the hook has disarmed itself: this one succeeds and replaces the keys
        engine.gate_batch(ol.OPS.index("NAND"), 0, dout, d0, d1, count=count)
        got = dout.download().reshape(count, -1)
        assert not np.array_equal(got, want_old)
        assert np.array_equal(got, other.gate_batch(ol.OPS.index("NAND"), 0, ins[0], ins[1]).reshape(count, -1))
    finally:
        api.set_option("test_fail_alloc", -1)
        engine.Initialize(keys.bk, keys.ksk)
    api.Synchronize()
    free2, _ = api.device_mem_info()
    assert abs(free0 - free2) < (32 << 20), "replacing the keys twice changed the device memory in use"


def test_empty_batch_and_errors(engine):
    api = engine.api
    buf = api.DeviceBuffer(ol.n + 1)
    api.gate_batch(0, 0, buf, buf, buf, count=0)          # no-op
    with pytest.raises(engine.CufheAmdError):
        api.gate_batch(99, 0, buf, buf, buf, count=1)      # unknown op
    with pytest.raises(engine.CufheAmdError):
        api.gate_batch(0, 2, buf, buf, buf, count=1)       # bad level
    with pytest.raises(engine.CufheAmdError):
        api.gate_batch(0, 0, buf, buf, None, count=1)      # missing operand


def test_two_levels_in_one_scheduler_batch(engine, keys):
    """lvl0 and lvl1 gates recorded together are launched in one flush (two launch sequences)."""
    api = engine.api
    st = api.Stream()
    st.Create()
    a0, b0, o0 = api.Ctxt(0), api.Ctxt(0), api.Ctxt(0)
    a1, b1, o1 = api.Ctxt(1), api.Ctxt(1), api.Ctxt(1)
    a0.tlwehost[:] = keys.encrypt([1], 0, seed=1)[0]; b0.tlwehost[:] = keys.encrypt([1], 0, seed=2)[0]
    a1.tlwehost[:] = keys.encrypt([0], 1, seed=3)[0]; b1.tlwehost[:] = keys.encrypt([1], 1, seed=4)[0]
    api.And(o0, a0, b0, st)
    api.OrNY(o1, a1, b1, st)
    api.Synchronize()
    assert keys.decrypt(o0.tlwehost, 0)[0] == 1 and keys.decrypt(o1.tlwehost, 1)[0] == 1
    st.Destroy()
