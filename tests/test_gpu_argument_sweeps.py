"""GPU sweeps of the two index-arithmetic kernel families the exponent sweep leaves out (tests/argument_sweeps.py holds the
references, tests/test_argument_sweeps.py pins them on the CPU):

  Spread     trlwe_spread_kernel at ALL 7262 (stride, reps) of cufhe_amd_trlwe_spread_batch, trlwe_spread_desc_kernel at all 66
             recorded pairs in one launch (and at 65: a workgroup with two dead waves)
  packing    the X^pos of pack_keyswitch_kernel's write-out at every pos in [0, N), alone in an output and all N in one output;
             the recorded pack at arity N, its documented limit, beside an arity-N pack of repeated handles and an arity-1 pack

Every test compares every output word, poisons its outputs before the call, keeps guard rows behind (recorded forms: around) the
outputs and checks them and the inputs unchanged.  A device error (status -2, a failed synchronize) ends the session: nothing
further is started on the device."""
import contextlib
import ctypes

import numpy as np
import pytest

import argument_sweeps as sw
import oracle_lib as ol
import pack_checker as pk
import pack_program_model as pm
import positions as ps
from cufhe_amd._lib import CufheAmdError

pytestmark = pytest.mark.gpu

N, n = ol.N, ol.n
ROW = 2 * N                              # words of a TRLWE
POISON = ps.POISON
SWEEP_SEED = 2400                        # tests/test_argument_sweeps.py pins spread_all on the same three TRLWEs
_cache = {}


def stop(label, rc, sync, lib):
    pytest.exit(f"{label}: status {rc}, synchronize {sync}: {lib.cufhe_amd_last_error().decode()}", returncode=3)


def synchronize(engine, label):
    sync = engine.lib.cufhe_amd_synchronize()
    if sync != 0:
        stop(label, 0, sync, engine.lib)


@contextlib.contextmanager
def device_errors_end_the_session(engine, label):
    """the object forms raise on a negative status: -2 (a HIP error) ends the session like a failed synchronize"""
    try:
        yield
    except CufheAmdError as e:
        if "error -2" in str(e):
            stop(label, -2, "not tried", engine.lib)
        raise


def up(engine, arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    return engine.api.DeviceBuffer(arr.size).upload(arr)


def reinit(engine, keys):
    engine.CleanUp()                     # (releases the packing key)
    engine.SetGPUNum(1)
    engine.Initialize(keys.bk, keys.ksk)


def guard_words(words, tag):
    """guard words that depend on their position and on the guard: a stray write of any constant, or of a neighbour's words, shows"""
    return ((np.arange(words, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(tag * 0x9E3779B1 + 0x5bd1e995)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


class Session:
    """streams and handles of one recorded test; TRLWE outputs are taken from handles sorted by device address, every second one, so
    that the handles around an output in that order are guards"""

    def __init__(self, engine, streams=2):
        self.engine, self.api, self.lib = engine, engine.api, engine.lib
        self.st = []
        for _ in range(streams):
            s = self.api.Stream()
            s.Create()
            self.st.append(s)

    def ctxt(self, words, k=0):
        c = self.api.Ctxt(0)
        c.tlwehost[:] = words
        self.api.CtxtCopyH2D(c, self.st[k % len(self.st)])
        return c

    def trlwe(self, words, k=0):
        t = self.api.Trlwe()
        t.trlwehost[:] = words
        self.api.CtxtCopyH2D(t, self.st[k % len(self.st)])
        return t

    def outputs_and_guards(self, count):
        ptr = lambda c: self.lib.cufhe_amd_ctxt_device_ptr(c._h, 0)
        ts = sorted((self.api.Trlwe() for _ in range(2 * count + 1)), key=ptr)
        outs, guards = ts[1::2], ts[0::2]
        for t in outs:
            t.trlwehost[:] = POISON
        for i, t in enumerate(guards):
            t.trlwehost[:] = guard_words(ROW, i)
        for t in ts:
            self.api.CtxtCopyH2D(t, self.st[0])
        return outs, guards

    def check_guards(self, guards):
        for i, t in enumerate(guards):
            assert np.array_equal(t.trlwehost, guard_words(ROW, i)), f"guard TRLWE {i} between the outputs was written"

    def close(self):
        for s in self.st:
            s.Destroy()


# ---- Spread: the batch kernel at every pair ----
def spread_inputs():
    if "x" not in _cache:
        _cache["x"] = sw.sweep_inputs(SWEEP_SEED)
    return _cache["x"]


def first_wrong_spread_word(got, want, pairs):
    """got, want [pairs][6][N]: None, or the message of the first wrong word"""
    if np.array_equal(got, want):
        return None
    bad = np.argwhere(got != want)
    i, poly, k = (int(v) for v in bad[0])
    wrong_pairs = sorted({pairs[int(j)] for j in np.unique(bad[:, 0])})
    return (f"{len(bad)} words differ in {len(wrong_pairs)} pairs (first pairs {wrong_pairs[:8]}); first: got {int(got[i, poly, k]):#x}, expected "
            f"{int(want[i, poly, k]):#x} at " + sw.describe_spread_failure(pairs[i][0], pairs[i][1], poly, k))


@pytest.mark.parametrize("band", sw.SPREAD_BANDS, ids=lambda b: f"stride{b[0]}-{b[1]}")
def test_spread_every_pair(engine, band):
    """one cufhe_amd_trlwe_spread_batch call of count = 3 per pair -- 6 polynomials: a full workgroup and one with two dead waves --
    each into its own rows of one output buffer: every word of every pair of the band equals spread_all"""
    lib = engine.lib
    x = spread_inputs()
    pairs = sw.spread_pairs(range(band[0], band[1] + 1))
    assert len(pairs) * 3 * ROW * 4 <= 32 << 20
    din = up(engine, x)
    dout = up(engine, ps.poison((len(pairs) * 3 + 1) * ROW))                # the last row is the guard
    for i, (stride, reps) in enumerate(pairs):
        rc = lib.cufhe_amd_trlwe_spread_batch(0, None, 3, din.ptr, stride, reps, dout.ptr + i * 3 * ROW * 4)
        if rc == -2:
            stop(f"Spread ({stride}, {reps})", rc, "not tried", lib)
        assert rc == 0, ((stride, reps), lib.cufhe_amd_last_error().decode())
    synchronize(engine, f"Spread, strides {band[0]} .. {band[1]}")
    got = dout.download()
    want = np.stack([w for _, w in sw.spread_all(x.reshape(6, N), range(band[0], band[1] + 1))])
    assert want.shape == (len(pairs), 6, N)
    assert np.all(got[-ROW:] == POISON), "the guard row behind the outputs was written"
    msg = first_wrong_spread_word(got[:-ROW].reshape(len(pairs), 6, N), want, pairs)
    assert msg is None, msg
    assert np.array_equal(din.download().reshape(3, ROW), x), "the inputs were written"


def test_spread_bands_cover_every_pair():
    """the bands of test_spread_every_pair together are the whole domain"""
    bands = [sw.spread_pairs(range(lo, hi + 1)) for lo, hi in sw.SPREAD_BANDS]
    assert sum(len(b) for b in bands) == 7262 and sorted(p for b in bands for p in b) == sorted(sw.spread_pairs())


# ---- Spread: the descriptor kernel at every recorded pair ----
def recorded_reference():
    """{pair: [6][N]} of the 66 recorded pairs on the three TRLWEs, once"""
    if "recorded" not in _cache:
        wanted = set(sw.recorded_spread_pairs())
        x = spread_inputs()
        _cache["recorded"] = {p: w for p, w in sw.spread_all(x.reshape(6, N), [1 << a for a in range(11)]) if p in wanted}
        assert len(_cache["recorded"]) == 66
    return _cache["recorded"]


@pytest.mark.parametrize("count", [66, 65])
def test_recorded_spread_every_pair(engine, count):
    """all 66 pairs with stride = 2^a, reps = 2^b, a + b <= 10 as gSpread from 3 input TRLWEs into distinct outputs in ONE dependence
    level and ONE launch: 33 workgroups of two TRLWEs whose descriptors differ in stride AND reps.  65 records: the last workgroup
    has two dead waves."""
    api = engine.api
    x, ref = spread_inputs(), recorded_reference()
    order = sw.recorded_spread_order(2500)[:count]
    assert len(set(order)) == count and all(a[0] != b[0] and a[1] != b[1] for a, b in zip(order, order[1:]))
    label = f"{count} recorded Spreads"
    S = Session(engine)
    with device_errors_end_the_session(engine, label):
        ins = [S.trlwe(x[g]) for g in range(3)]
        outs, guards = S.outputs_and_guards(count)
        api.Synchronize()                    # operands are on the device: what follows is the Spreads alone
        api.sched_stats(reset=True)
        for k, (stride, reps) in enumerate(order):
            api.gSpread(outs[k], ins[k % 3], stride, reps, S.st[k % 2])
        for t in outs + guards + ins:
            api.CtxtCopyD2H(t, S.st[0])
        synchronize(engine, label)
        stats = api.sched_stats()
    assert stats.gates == count and stats.levels == 1 and stats.launch_sequences == 1, (stats.gates, stats.levels, stats.launch_sequences)
    for k, (stride, reps) in enumerate(order):
        g = k % 3
        want = ref[(stride, reps)][2 * g:2 * g + 2]
        got = outs[k].trlwehost.reshape(2, N)
        if not np.array_equal(got, want):
            j, c = (int(v) for v in np.argwhere(got != want)[0])
            pytest.fail(f"record {k} (workgroup {k // 2}, its TRLWE {k % 2}; the neighbour's pair {order[k ^ 1] if (k ^ 1) < count else None}): "
                        f"{int((got != want).sum())} words differ; first: got {int(got[j, c]):#x}, expected {int(want[j, c]):#x} at "
                        + sw.describe_spread_failure(stride, reps, 2 * k + j, c))
    S.check_guards(guards)
    assert all(np.array_equal(ins[g].trlwehost, x[g]) for g in range(3)), "the inputs were written"
    S.close()


# ---- packing ----
def pack_rows():
    """the 7 distinct lvl0 inputs of the packing sweeps (edge words of the digit decomposition sown in), the random key and the model
    that computes PackKS once per distinct input"""
    if "pack" not in _cache:
        key = np.random.default_rng(900).integers(0, 1 << 32, size=pk.KEY_WORDS, dtype=np.uint64).astype(np.uint32)
        x7 = pk.edge_inputs(np.random.default_rng(2600), sw.PACK_ROWS)
        model = pm.Model(key)
        _cache["pack"] = (x7, key, model, np.stack([model.pack_ks(x7[i]) for i in range(sw.PACK_ROWS)]))
    return _cache["pack"]


@pytest.fixture(scope="module")
def pack_engine(engine, keys):
    """the engine with the random packing key loaded (word parity needs no genuine key); a freshly initialised engine without a
    packing key for the files that follow"""
    engine.api.pack_initialize(pack_rows()[1])
    yield engine
    reinit(engine, keys)


def describe_pack_failure(got, want, dst, pos):
    bad = np.argwhere(got != want)
    o, w = (int(v) for v in bad[0])
    terms = np.flatnonzero(dst == o)
    text = f"{len(bad)} words differ in outputs {sorted(set(bad[:, 0].tolist()))[:8]}; first at output {o}, polynomial {w // N}, coefficient {w % N}"
    if len(terms) == 1:
        m, p = int(terms[0]), int(pos[terms[0]])
        k = (w % N - p) % N
        text += (f": its one term is input {m} (row {m % sw.PACK_ROWS}, tile {m // 64} slot {m % 64}) at pos {p}; the word comes from row "
                 f"coefficient k = {k}, k + pos = {k + p}{' (wraps: negated)' if k + p >= N else ''}")
    return text + f": got {int(got[o, w]):#x}, expected {int(want[o, w]):#x}"


@pytest.mark.parametrize("which", ["isolated", "shared"])
def test_pack_every_position(pack_engine, which):
    """count = N + 1 = 1025 inputs tiled from 7 rows -- sixteen full tiles and a tile of one -- at "pack_slices" 1, 40 and the
    automatic rule.  isolated: dst[m] = m, pos[m] = m mod N, every position alone in its output.  shared: output 0 receives N terms at
    a permutation of 0 .. N - 1, output 1 the remaining term."""
    engine, api, lib = pack_engine, pack_engine.api, pack_engine.lib
    x7, key, model, rows = pack_rows()
    count = N + 1
    dst, pos, count_out = sw.pack_targets(2403)[which]
    x = ps.tile(x7, count)
    want = np.zeros((count_out, ROW), np.uint32)
    for m in range(count):
        want[dst[m]] += pk.rotate(rows[m % sw.PACK_ROWS], int(pos[m]))      # uint32 wraps
    din = up(engine, x)
    dout = api.DeviceBuffer((count_out + 1) * ROW)                          # the last row is the guard
    try:
        for slices in (1, 40, -1):
            api.set_option("pack_slices", slices)
            dout.upload(ps.poison((count_out + 1) * ROW))
            rc = lib.cufhe_amd_pack_batch(0, None, count, din.ptr, dst.ctypes.data, pos.ctypes.data, count_out, dout.ptr)
            if rc == -2:
                stop(f"pack_batch, {which}, pack_slices {slices}", rc, "not tried", lib)
            assert rc == 0, lib.cufhe_amd_last_error().decode()
            synchronize(engine, f"pack_batch, {which}, pack_slices {slices}")
            got = dout.download().reshape(count_out + 1, ROW)
            assert np.all(got[-1] == POISON), f"pack_slices {slices}: the guard row behind the outputs was written"
            assert np.array_equal(got[:-1], want), f"pack_slices {slices}: " + describe_pack_failure(got[:-1], want, dst, pos)
    finally:
        api.set_option("pack_slices", -1)
    assert np.array_equal(din.download().reshape(count, n + 1), x), "the inputs were written"


@pytest.mark.parametrize("rename", [0, 1])
def test_recorded_pack_at_full_arity(pack_engine, keys, rename):
    """one dependence level: a gPack of arity N from 1024 distinct handles at permuted positions, a second of arity N from 7 handles
    repeated, all at position 1023, and an arity-1 pack at position 0 -- 2049 terms, one zeroing launch and one key-switch launch.  Then
    arity N + 1 is refused and records nothing; then a NAND overwrites input 777 and an arity-N pack of the same handles follows with
    no fence: its words use the NAND's output."""
    engine, api, lib = pack_engine, pack_engine.api, pack_engine.lib
    x7, key, model, rows = pack_rows()
    tdst, tpos, _ = sw.pack_targets(2403)["shared"]
    perm = tpos[tdst == 0]
    assert sorted(perm.tolist()) == list(range(N))
    words = [x7[i % sw.PACK_ROWS] for i in range(N)]
    label = f"recorded packs of arity {N}, sched_rename {rename}"
    S = Session(engine)
    api.set_option("sched_rename", rename)
    try:
        with device_errors_end_the_session(engine, label):
            handles = [S.ctxt(words[i], i) for i in range(N)]
            ga, gb = S.ctxt(x7[3]), S.ctxt(x7[5])
            (out_all, out_rep, out_one, out_dep), guards = S.outputs_and_guards(4)
            api.Synchronize()
            packs = [(out_all, list(range(N)), perm),
                     (out_rep, [m % sw.PACK_ROWS for m in range(N)], np.full(N, N - 1, np.int32)),
                     (out_one, [9], np.zeros(1, np.int32))]
            api.sched_stats(reset=True)
            api.profile_enable(True)
            try:
                api.profile_get(reset=True)
                for k, (out, idx, pos) in enumerate(packs):
                    api.gPack(out, [handles[i] for i in idx], pos, S.st[k % 2])
                for c in [out_all, out_rep, out_one] + guards + handles:
                    api.CtxtCopyD2H(c, S.st[0])
                synchronize(engine, label)
                stats = api.sched_stats()
                prof = api.profile_get(reset=True)
            finally:
                api.profile_enable(False)
            for k, (out, idx, pos) in enumerate(packs):
                want = model.pack([words[i] for i in idx], pos)
                bad = np.flatnonzero(out.trlwehost != want)
                assert bad.size == 0, f"pack {k} of arity {len(idx)}: {bad.size} words differ, first at polynomial {int(bad[0]) // N}, coefficient {int(bad[0]) % N}"
            assert stats.gates == 3 and stats.levels == 1, (stats.gates, stats.levels)
            # one pack lowering over all 2049 terms: a single profiled launcher call (the zeroing launch and the key-switch launch), no rotation
            assert (prof.keyswitch_launches, prof.keyswitches) == (1, 2 * N + 1), (prof.keyswitch_launches, prof.keyswitches)
            assert prof.blind_rotate_launches == 0
            S.check_guards(guards)
            assert all(np.array_equal(handles[i].tlwehost, words[i]) for i in range(N)), "the inputs were written"

            # arity N + 1: refused, nothing recorded
            before = int(api.sched_stats().gates)
            arr = (ctypes.c_void_p * (N + 1))(*[handles[i % N]._h for i in range(N + 1)])
            p = np.zeros(N + 1, np.int32)
            assert lib.cufhe_amd_enqueue_pack(0, S.st[0].st(), 0, out_dep._h, N + 1, arr, p.ctypes.data) == -1
            assert b"count_in" in lib.cufhe_amd_last_error(), lib.cufhe_amd_last_error()
            assert int(api.sched_stats().gates) == before

            # a gate writes input 777 (an input beyond the third: entered by record_pack itself), the pack follows with no fence
            api.gNand(handles[777], ga, gb, S.st[0])
            api.gPack(out_dep, handles, perm, S.st[1])
            for c in [out_dep, handles[777], handles[776], handles[778]] + guards:
                api.CtxtCopyD2H(c, S.st[1])
            synchronize(engine, label + ", the dependent pack")
        nand = keys.gate_batch(api.NAND, 0, x7[3][None, :], x7[5][None, :])[0]
        assert np.array_equal(handles[777].tlwehost, nand) and not np.array_equal(nand, words[777])
        assert np.array_equal(handles[776].tlwehost, words[776]) and np.array_equal(handles[778].tlwehost, words[778])
        after = list(words)
        after[777] = nand
        want = model.pack(after, perm)
        stale = model.pack(words, perm)
        assert not np.array_equal(want, stale)
        got = out_dep.trlwehost
        assert not np.array_equal(got, stale), "the pack read input 777 before the NAND wrote it"
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"dependent pack: {bad.size} words differ, first at polynomial {int(bad[0]) // N}, coefficient {int(bad[0]) % N}"
        assert np.all(out_all.trlwehost == model.pack(words, perm))
        S.check_guards(guards)
    finally:
        api.set_option("sched_rename", 1)
    S.close()
