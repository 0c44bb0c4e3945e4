"""Random programs over EVERY kind of record the per-gate API makes, on the real device, against the in-order model of
tests/program_model.py (whose CPU test is tests/test_program_model.py; the CPU twin with a stubbed device is the random program of
tests/host/sched_harness.cpp).

What is under test is ORDER: which value every recorded read sees and every host member ends up with, when user gates, multi-output
evaluations (together and sibling by sibling), the TRLWE-level operations, SEIKS_AT, CMUXNTT, in-place CMUXRotateNTT chains, circuit
bootstraps into TRGSW holders, TRGSW2NTT, copies, polls, Flush and Synchronize meet in one dependent program.  Every kernel on the way is
pinned word for word elsewhere; here every observed word is compared with the value of the in-order DAG, computed on the CPU by the
checkers the suite already has -- with one exception: the value of a circuit bootstrap node comes from ONE call of
circuit_bootstrap_batch on the node's input words (the Python checker costs about 11.6 s per input; that entry point is pinned to it by
tests/test_gpu_circuit_bootstrap.py and tests/test_gpu_positions.py), made after the program's last Synchronize.  Likewise the NTT image of a
TRGSW2NTT value is what the library itself wrote to the holder's host member at the call: for such a holder the comparison shows that
nothing overwrote or tore those words, not that the transform is right (tests/test_gpu_positions.py pins it); the selector's TORUS
words enter the CMUX checkers independently.

Modes: "a" the default ring with every kind, "sched_rename" 0 and 1; "b" the netlist form with "sched_two_lane" 2 and "cus_override" 16;
"c" "lvl0_ring" 2048: built-in gates, lvl2 user gates and CUFHE_AMD_LVL2_USER_OP_OUTPUT siblings one by one, against
lvl2_user_gate_checker / lvl2_multi_checker; "d" "param_set" on k2n512 and cggi16: gates of both levels, the set's user ops and siblings,
TL_BOOTSTRAP / REFRESH / SEIKS, CMUXNTT, TRGSW2NTT and copies, against ps_user_gate_checker and the set's oracle.  The same recorded
program lowers to other kernels there, with their own user-op ranges and their own sibling grouping.
A flush that holds an output of a multi-output gate is never scheduled gate by gate (compile_two_lane refuses it: such outputs share a
rotation only inside one launch, Backend::shares_rotation), so a netlist has two parts: built-in and single-output user gates, which
must take the two-lane path, then the same with multi-output evaluations, level by level.
"""
import time
import types

import numpy as np
import pytest

import cb_checker as cb
import oracle_lib as ol
import program_model as pm
import ps_user_gate_checker as pc

pytestmark = pytest.mark.gpu

N, n = ol.N, ol.n


@pytest.fixture(scope="module")
def world(engine, keys, oracle):
    """a freshly initialised engine with the lvl02 key, a private key-switching key of random words (word checks need no encryption) and
    the user gates of program_model.user_defs(); the session's state again afterwards"""
    keys2 = ol.KeysLvl2(oracle, keys, seed=7)
    engine.CleanUp()
    engine.SetGPUNum(1)
    engine.Initialize(keys.bk, keys.ksk)
    engine.lvl2_initialize(keys2.bk, keys2.ksk)
    engine.api.cb_initialize(np.random.default_rng(2024).integers(0, 2**32, size=cb.PKS_KEY_WORDS, dtype=np.uint32))
    ops = [engine.define_gate(c, off, tv, nout=nout) for c, off, tv, nout in pm.user_defs()]
    ring = pm.Env("ring", keys2=keys2)
    ring.ops = [engine.lvl2_define_gate(c, off, tv, nout=nout) for c, off, tv, nout in ring.defs]
    yield types.SimpleNamespace(engine=engine, ops=ops, ring=ring)
    engine.CleanUp()
    engine.SetGPUNum(1)
    engine.Initialize(keys.bk, keys.ksk)


def cb_oracle(api):
    def f(words):
        count = len(words)
        d0 = api.DeviceBuffer(count * (n + 1)).upload(np.ascontiguousarray(np.stack(words), np.uint32))
        dt = api.DeviceBuffer(count * cb.TRGSW_WORDS)
        dn = api.DeviceBuffer(count * cb.TRGSW_WORDS * 2)
        api.circuit_bootstrap_batch(d0, count, trgsw=dt, trgsw_ntt=dn)
        torus, ntt = dt.download().reshape(count, -1), dn.download().reshape(count, -1)
        return [(torus[g].copy(), ntt[g].copy()) for g in range(count)]
    return f


@pytest.fixture(scope="module", params=["k2n512", "cggi16"])
def on_set(request, world):
    """a compiled parameter set beside the default keys: its checker and keys, its keys on the device, its user gates"""
    api = world.engine.api
    env = pm.Env("set", checker=pc.Checker(request.param, seed=5))
    env.idx = api.ps_index(request.param)
    api.ps_initialize(env.idx, env.C.K.bk, env.C.K.ksk)
    env.ops = [api.ps_define_gate(env.idx, c, off, tv, nout=nout) for c, off, tv, nout in env.defs]
    return env


def run(engine, ops, keys, m, env=None):
    api = engine.api
    t0 = time.time()
    ct, obs, ntt = pm.issue(api, m, ops, env)
    t1 = time.time()
    val = pm.evaluate(m, {v for _, _, _, v in obs}, keys, cb_oracle=cb_oracle(api), env=env)
    print("\n%d records issued in %.2f s, %d observations, %d values computed in %.2f s; hazards %s" % (
        len(m.records), t1 - t0, len(obs), len(val), time.time() - t1, dict(sorted(m.hazards.items()))))
    msg = pm.compare(m, obs, ntt, val)
    assert msg is None, msg
    return obs


@pytest.mark.parametrize("seed", pm.seeds("a"))
@pytest.mark.parametrize("rename", [0, 1])
def test_every_kind_matches_the_in_order_model(world, keys, rename, seed):
    """mode (a): about 120 records of every kind on 10 lvl0, 5 lvl1, 5 TRLWE ciphertexts and 3 TRGSW holders over 5 streams; every host
    member after each Synchronize, after each StreamQuery that returned true, and at the end"""
    engine, ops = world.engine, world.ops
    engine.api.set_option("sched_rename", rename)
    try:
        obs = run(engine, ops, keys, pm.generate("a", seed))
    finally:
        engine.api.set_option("sched_rename", 1)
    assert any(label.startswith("after StreamQuery") for label, _, _, _ in obs) and any(x[0] == 3 for _, x, _, _ in obs)


@pytest.mark.parametrize("seed", pm.seeds("b"))
def test_netlist_with_user_and_multi_output_gates_on_two_lanes(world, keys, seed):
    """mode (b): device-resident built-in gates and single-output user gates scheduled gate by gate on two lanes, then a part with
    multi-output evaluations, which the level order keeps; every value fetched"""
    engine, ops = world.engine, world.ops
    api = engine.api
    api.set_option("cus_override", 16)
    api.set_option("sched_two_lane", 2)
    try:
        api.Synchronize()
        api.sched_stats(reset=True)
        run(engine, ops, keys, pm.generate("b", seed))
        stats = api.sched_stats()
        assert stats.two_lane_groups >= 1 and stats.two_lane_launches >= 2, (stats.two_lane_groups, stats.two_lane_launches, stats.levels)
    finally:
        api.set_option("sched_two_lane", 1)
        api.set_option("cus_override", 0)


@pytest.mark.parametrize("seed", pm.seeds("c"))
def test_ring_2048_programs_match_the_in_order_model(world, keys, seed):
    """mode (c), "lvl0_ring" 2048: built-in gates, a lvl2 user gate, and the outputs of one multi-output definition recorded one by one
    (CUFHE_AMD_LVL2_USER_OP_OUTPUT) in shuffled order on changing streams, with nothing, a write to an operand or a Flush between them,
    copying and then device-resident, every value fetched.  An evaluation costs the ring's Python checker about 2 s, one after the
    other, which sets this test's time: a program holds two (the operand is written once), the first seed a single-output user gate
    besides."""
    api = world.engine.api
    api.set_option("lvl0_ring", 2048)
    try:
        run(world.engine, world.ring.ops, keys, pm.generate("c", seed), world.ring)
    finally:
        api.set_option("lvl0_ring", 1024)


@pytest.mark.parametrize("seed", pm.seeds("d"))
def test_parameter_set_programs_match_the_in_order_model(world, on_set, keys, seed):
    """mode (d), "param_set" on k2n512 (k = 2, N = 512) and cggi16 (two key limbs): about 65 records -- gates of both levels, the set's user
    gates and sibling outputs (CUFHE_AMD_PS_USER_OP_OUTPUT, one by one), TL_BOOTSTRAP / REFRESH / SEIKS, CMUXNTT (also in place),
    TRGSW2NTT of steps of the set's bootstrapping key, copies, polls, Flush, Synchronize and host edits"""
    api = world.engine.api
    api.set_option("param_set", on_set.idx)
    try:
        run(world.engine, on_set.ops, keys, pm.generate("d", seed, on_set.level_words), on_set)
    finally:
        api.set_option("param_set", -1)


def test_multi_output_evaluation_with_a_raw_stream_handle_out(world, keys):
    """Found by the random programs of the stub harness (group_with_raw_handle_out there): once a stream's raw handle is out every copying
    gate uploads its operands anew, and the eight outputs of ONE ApplyMulti did so one after the other, each behind the sibling before it --
    eight levels, eight rotations.  One upload, one level, the checker's words."""
    engine, ops = world.engine, world.ops
    api = engine.api
    st = api.Stream()
    st.Create()
    rng = np.random.default_rng(31)
    m = pm.Model({0: 12, 1: 0, 2: 0, 3: 0}, rng)
    api.Synchronize()
    engine.check(engine.lib.cufhe_amd_stream_fence(0, st.st()))
    api.sched_stats(reset=True)
    m.apply(("multi", 5, True, tuple((0, 3 + j) for j in range(8)), ((0, 0), (0, 1), (0, 2)), 0))
    m.apply(("sync",))
    try:
        ct, obs, ntt = pm.issue(api, m, ops)
        stats = api.sched_stats()
    finally:
        st.Destroy()            # (the handle leaves the scheduler's books with its stream, whatever happened)
    assert stats.gates == 8 and stats.levels == 1 and stats.launch_sequences == 1, (stats.gates, stats.levels, stats.launch_sequences)
    msg = pm.compare(m, obs, ntt, pm.evaluate(m, {v for _, _, _, v in obs}, keys))
    assert msg is None, msg


def test_delivery_stays_behind_a_recorded_upload_of_the_same_host_words(world, keys):
    """Found by the random programs of the stub harness (delivery_ahead_of_upload there, where a held launch worker makes it
    deterministic): a copying gate reads c, its upload of c's tlwehost sitting behind the device-resident gates that wrote c's buffer;
    a copying gate on another stream then overwrites c and, renamed, sits in the front level; its stream is polled until the result has
    arrived in c's tlwehost.  The first gate must have read the words from before.
    NOT a guard: on the device this depends on the launch worker being slower than the poll, and the unfixed scheduler usually passes
    it.  The deterministic pin is delivery_ahead_of_upload of the stub harness; this is the same program on the real device."""
    engine, ops = world.engine, world.ops
    api = engine.api
    m = pm.Model({0: 5, 1: 0, 2: 0, 3: 0}, np.random.default_rng(32))
    c, x, y, z, r = [(0, i) for i in range(5)]
    for rec in [("h2d", c, 0), ("h2d", x, 0), ("gate", "AND", False, c, (c, x), 0), ("gate", "OR", False, c, (c, x), 0),
                ("gate", "XOR", False, c, (c, x), 0), ("gate", "XOR", True, r, (c, y), 0), ("gate", "OR", True, c, (y, z), 1), ("wait", 1), ("sync",)]:
        m.apply(rec)
    ct, obs, ntt = pm.issue(api, m, ops)
    msg = pm.compare(m, obs, ntt, pm.evaluate(m, {v for _, _, _, v in obs}, keys))
    assert msg is None, msg
