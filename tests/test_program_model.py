"""tests/program_model.py without a device: on fixed straight-line programs the model's values are what direct calls of the checkers
give, copying and device-resident forms follow the reference's host / device semantics, and the committed seeds of every mode contain
every hazard class the mode can express at least 3 times (the condition that keeps a seed from hiding a gap, profiles/r22_random_programs.md)."""
import numpy as np
import pytest

import multi_output_checker as mc
import oracle_lib as ol
import packed_rom_checker as pr
import program_model as pm
import user_gate_checker as uc

N, n = ol.N, ol.n


def fake_cb(words):
    """a stand-in for the circuit bootstrap (the real one is a GPU call): torus and NTT words that depend on every input word"""
    out = []
    for w in words:
        rng = np.random.default_rng([int(x) for x in w[:8]] + [int(np.bitwise_xor.reduce(w))])
        out.append((rng.integers(0, 1 << 32, size=pm.TRGSW_WORDS, dtype=np.uint64).astype(np.uint32),
                    rng.integers(0, 1 << 32, size=4 * pm.TRGSW_WORDS, dtype=np.uint64).astype(np.uint32)))
    return out


SET_WORDS = {0: 631, 1: 1025, 2: 1536}          # k2n512's; the records of mode (d) do not depend on the word counts


@pytest.mark.parametrize("mode,classes", [("a", pm.CLASSES_A), ("b", pm.CLASSES_B), ("c", pm.CLASSES_C), ("d", pm.CLASSES_D)])
def test_committed_seeds_contain_every_hazard_class(mode, classes):
    total = {}
    for seed in pm.SEEDS[mode]:
        m = pm.generate(mode, seed, SET_WORDS if mode == "d" else None)
        assert (100 if mode in "ab" else 20) <= len(m.records) <= 180
        if mode == "d":
            assert [r[0] for r in m.records] == [r[0] for r in pm.generate("d", seed, {0: 501, 1: 1025, 2: 2048}).records]
        for k, v in m.hazards.items():
            total[k] = total.get(k, 0) + v
    print(mode, {c: total.get(c, 0) for c in classes})
    missing = {c: total.get(c, 0) for c in classes if total.get(c, 0) < 3}
    assert not missing, missing


def test_generation_is_deterministic():
    a, b = pm.generate("a", 1), pm.generate("a", 1)
    assert len(a.records) == len(b.records) and a.hazards == b.hazards
    assert [r[0] for r in a.records] == [r[0] for r in b.records]


def test_straight_line_program_equals_direct_checker_calls(keys):
    """one record of every kind, copying and device-resident, on a small pool: every value the model holds at the end is the value of
    the direct checker call on the operands' values"""
    L = keys.L
    rng = np.random.default_rng(5)
    m = pm.Model({0: 4, 1: 3, 2: 3, 3: 2}, rng)
    defs = pm.user_defs()
    init = {x: m.nodes[m.host[x]][1] for x in m.names if x[0] != 3}
    tg = rng.integers(0, 1 << 32, size=pm.TRGSW_WORDS, dtype=np.uint64).astype(np.uint32)
    a, b, c, d = [(0, i) for i in range(4)]
    p, q, r = [(1, i) for i in range(3)]
    t0, t1, t2 = [(2, i) for i in range(3)]
    h0, h1 = (3, 0), (3, 1)
    prog = [("ntt", h0, tg, 0),
            ("gate", "XOR", True, c, (a, b), 0),                 # c = XOR(a, b), host and device
            ("user", 1, False, d, (c, a), 1),                    # device only: d's host keeps its initial words
            ("multi", 3, True, (p, q), (r,), 2),                 # two outputs of one evaluation on one lvl1 operand
            ("boot", False, t0, c, 0),
            ("refresh", True, t1, t1, 1),                        # copying, in place: from t1's host words
            ("cb", False, h1, d, 3),
            ("cmux", False, t2, h0, t0, t0, 0),                  # c1 == c0
            ("h2d", t1, 0),
            ("cmux", False, t0, h1, t0, t1, 1),                  # in place on c1, selector from the circuit bootstrap
            ("cmuxrot", 1025, False, t0, h0, t0, 2),
            ("seiks_at", 64, False, a, t0, 0),
            ("seiks_at", 0, True, b, t1, 0),
            ("d2h", a, 4), ("d2h", d, 4), ("d2h", t0, 4), ("d2h", t2, 4), ("d2h", h1, 4),
            ("sync",)]
    for rec in prog:
        m.apply(rec)
    snap = m.records[-1][1]
    val = pm.evaluate(m, snap.values(), keys, cb_oracle=fake_cb, threads=4)
    w_c = keys.gate_batch(ol.OPS.index("XOR"), 0, init[a].reshape(1, -1), init[b].reshape(1, -1))[0]
    w_d = uc.user_gate_one(keys, 0, defs[1][0], defs[1][1], defs[1][2], [w_c, init[a]])
    md = 3
    w_pq = mc.multi_gate_one(keys, 1, defs[md][0], defs[md][1], defs[md][2], defs[md][3], [init[r]])
    w_t0 = keys.blind_rotate(w_c)
    w_t1 = np.zeros(2 * N, np.uint32)
    L.orc_refresh(keys.ek, w_t1, init[t1])
    w_h1 = fake_cb([w_d])[0]
    w_t2 = pr.cmux(L, tg, w_t0, w_t0)
    w_t0 = pr.cmux(L, w_h1[0], w_t0, w_t1)
    w_t0 = pr.cmux_rotate(L, tg, w_t0, 1025)
    w_a = pr.extract_keyswitch(keys, w_t0, 64)
    w_b = np.zeros(n + 1, np.uint32)
    L.orc_sample_extract_keyswitch(keys.ek, w_b, w_t1)
    want = {a: w_a, b: w_b, c: w_c, d: w_d, p: w_pq[0], q: w_pq[1], r: init[r], t0: w_t0, t1: w_t1, t2: w_t2}
    for x, w in want.items():
        assert np.array_equal(val[snap[x]], w), (x, pm.describe(m, snap[x]))
    assert np.array_equal(val[snap[h1]][1], w_h1[1]) and m.nodes[snap[h0]][0] == "trgsw"
    # the comparison names the record that made the value and the producers of its operands
    obs = [("at the end", x, want[x].copy(), snap[x]) for x in want]
    assert pm.compare(m, obs, {}, val) is None
    obs[0][2][3] ^= 1
    msg = pm.compare(m, obs, {}, val)
    assert "ciphertext (0, 0)" in msg and "made by record #11" in msg and "operand value" in msg and "made by record #10" in msg, msg


def test_g_forms_leave_the_host_member_alone(keys):
    rng = np.random.default_rng(6)
    m = pm.Model({0: 3, 1: 0, 2: 0, 3: 0}, rng)
    a, b, c = [(0, i) for i in range(3)]
    h = dict(m.host)
    m.apply(("h2d", a, 0))
    m.apply(("h2d", b, 0))
    m.apply(("gate", "AND", False, c, (a, b), 0))
    assert m.host[c] == h[c] and m.dev[c] != h[c]
    m.apply(("edit", a, rng.integers(0, 1 << 32, size=n + 1, dtype=np.uint64).astype(np.uint32)))
    m.apply(("gate", "OR", False, b, (a, c), 0))                  # reads a's DEVICE value: the words from before the edit
    assert m.nodes[m.dev[b]][2][0] == h[a]
    m.apply(("gate", "OR", True, b, (a, c), 0))                   # the copying form uploads both operands' host members
    assert m.nodes[m.dev[b]][2] == (m.host[a], h[c]) and m.host[b] == m.dev[b]


def test_parameter_set_values_equal_direct_checker_calls():
    """mode (d) on k2n512: the set's gates, user gate, sibling outputs, TRLWE-level ops and CMUXNTT through `evaluate` are the direct calls
    of ps_user_gate_checker.Checker and the set's oracle"""
    import ps_user_gate_checker as pc
    env = pm.Env("set", checker=pc.Checker("k2n512", seed=5))
    C, K, L = env.C, env.C.K, env.C.L
    m = pm.Model({0: 4, 1: 2, 2: 2, 3: 1}, np.random.default_rng(8), env.level_words)
    init = {x: m.nodes[m.host[x]][1] for x in m.names if x[0] != 3}
    a, b, c, d = [(0, i) for i in range(4)]
    p, q = (1, 0), (1, 1)
    t0, t1 = (2, 0), (2, 1)
    for rec in [("ntt", (3, 0), 5, 0), ("gate", "NOR", True, c, (a, b), 0), ("sib", 4, 2, True, d, (c, a), 1), ("user", 0, True, q, (p,), 1),
                ("boot", False, t0, c, 0), ("refresh", True, t1, t1, 1), ("cmux", False, t0, (3, 0), t0, t1, 0), ("seiks_at", 0, False, a, t0, 0),
                ("d2h", a, 0), ("d2h", t0, 0), ("sync",)]:
        m.apply(rec)
    snap = m.records[-1][1]
    val = pm.evaluate(m, snap.values(), None, env=env, threads=4)
    defs = env.defs
    w_c = K.gate_batch(ol.OPS.index("NOR"), 0, init[a][None, :], init[b][None, :])[0]
    w_d = C.user_gate_one(0, defs[4][0], defs[4][1], defs[4][2], [w_c, init[a]], s=2)[2]
    w_q = C.user_gate_one(1, defs[0][0], defs[0][1], defs[0][2], [init[p]])[0]
    se = np.zeros(C.words[1], np.uint32)
    L.orc_sample_extract0(se, init[t1])
    w_t1 = K.blind_rotate(K.keyswitch(se))
    w_t0 = np.zeros(C.acc_words, np.uint32)
    L.orc_cmux(w_t0, env.trgsw(5), K.blind_rotate(w_c), w_t1)
    assert np.array_equal(C.sample_extract(w_t0, 0), (L.orc_sample_extract0(se, w_t0), se)[1])      # the checker's own extraction agrees
    w_a = K.keyswitch(C.sample_extract(w_t0, 0))
    for x, w in {c: w_c, d: w_d, q: w_q, t1: w_t1, t0: w_t0, a: w_a}.items():
        assert np.array_equal(val[snap[x]], w), (x, pm.describe(m, snap[x]))


def test_ring_values_equal_direct_checker_calls(oracle, keys):
    """mode (c): a built-in gate and one sibling output on the N = 2048 ring through `evaluate` are the direct calls of the ring's
    oracle and of lvl2_multi_checker"""
    import lvl2_multi_checker as mc2
    keys2 = ol.KeysLvl2(oracle, keys, seed=7)
    env = pm.Env("ring", keys2=keys2)
    m = pm.Model({0: 4, 1: 0, 2: 0, 3: 0}, np.random.default_rng(9))
    init = {x: m.nodes[m.host[x]][1] for x in m.names}
    a, b, c, d = [(0, i) for i in range(4)]
    for rec in [("gate", "XNOR", True, c, (a, b), 0), ("sib", 3, 1, True, d, (c,), 1), ("sync",)]:
        m.apply(rec)
    snap = m.records[-1][1]
    val = pm.evaluate(m, snap.values(), keys, env=env, threads=2)
    w_c = keys2.gate_batch(np.array([ol.OPS.index("XNOR")], np.int32), init[a][None, :], init[b][None, :], None, threads=1)[0]
    dd = env.defs[3]
    w_d = keys2.keyswitch(mc2.multi_extract_one(keys2, dd[0], dd[1], dd[2], dd[3], [w_c])[1])
    assert np.array_equal(val[snap[c]], w_c) and np.array_equal(val[snap[d]], w_d)
