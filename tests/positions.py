"""Every output word at every batch position: helpers of tests/test_positions.py and tests/test_gpu_positions.py.

A batch of `count` rows is built from D distinct inputs, row g carrying input g % D.  D is a prime that divides no grouping of
the kernels (8, 12 or 16 rotations / ciphertexts per workgroup, 64, 2048, the CU counts), so neighbouring rows always differ
and the period drifts through every slot of every grouping: the reference is computed once per distinct input and ALL rows
are compared with it, no sample.
"""
import contextlib

import numpy as np

POISON = 0xDEADBEEF
GROUPINGS = (8, 12, 16, 64, 2048, 256, 40, 104)       # rotations / ciphertexts per workgroup, a default grid round, CU counts in play
PRIMES = (7, 11, 17, 19, 23, 59, 61, 67)

# cufhe_amd_set_option keys a test may change, with the value that restores the library's default
OPTION_DEFAULTS = {
    "ll_threshold": -1, "ll2_threshold": -1, "half_threshold": -1, "tail_split": 1,
    "ks_wg_threshold": -1, "ks_split_threshold": -1, "ks_per_wg": -1, "ks_slices": -1,
    "ps_batch_threshold": -1, "lvl2_kernel": -1, "lvl0_ring": 1024, "cus_override": 0,
    "param_set": -1, "sched_zero_copy": 1, "sched_rename": 1,
    "br_shape": 0, "ks_mm_threshold": -1, "cb_rotations": 3,         # "br_shape" is the calling thread's own
}


def check_period(D, groupings=GROUPINGS):
    """D must be a prime that divides none of the groupings"""
    assert D >= 2 and all(D % p for p in range(2, int(D ** 0.5) + 1)), f"period {D} is not a prime"
    for m in groupings:
        assert m % D, f"period {D} divides the grouping {m}: the rows would not drift through its slots"


def tile(distinct, count):
    """[count, ...]: row g carries distinct[g % D]"""
    distinct = np.asarray(distinct)
    check_period(distinct.shape[0])
    return np.ascontiguousarray(distinct[np.arange(count) % distinct.shape[0]])


def poison(shape, dtype=np.uint32):
    """what an output buffer holds before a launch: a row nobody wrote is a mismatch"""
    if np.dtype(dtype) == np.uint64:
        return np.full(shape, (POISON << 32) | POISON, np.uint64)
    return np.full(shape, POISON, dtype)


def residues_visited(D, count, m):
    """the set of (g % D, g % m) over the rows of a tiled batch"""
    g = np.arange(count)
    return set(zip((g % D).tolist(), (g % m).tolist()))


def every_input_visits_every_slot(D, count, m):
    """True when each of the D distinct inputs lands on each of the m slots within `count` rows (needs count >= D m: CRT)"""
    return len(residues_visited(D, count, m)) == D * m


def every_slot_is_visited(D, count, m):
    """True when the rows of the batch cover every slot of the grouping and every distinct input"""
    seen = residues_visited(D, count, m)
    return {d for d, _ in seen} == set(range(min(D, count))) and {s for _, s in seen} == set(range(min(m, count)))


def report(got, want_distinct, label, groupings=()):
    """None if row g of `got` equals want_distinct[g % D] for every g, else the failure message"""
    got = np.asarray(got)
    want_distinct = np.asarray(want_distinct)
    D = want_distinct.shape[0]
    check_period(D)
    count = got.shape[0]
    if got.dtype != want_distinct.dtype or got.shape[1:] != want_distinct.shape[1:]:
        return f"{label}: got rows of {got.dtype}{got.shape[1:]}, expected {want_distinct.dtype}{want_distinct.shape[1:]}"
    got2 = got.reshape(count, -1)
    dist2 = want_distinct.reshape(D, -1)
    want = dist2[np.arange(count) % D]
    if np.array_equal(got2, want):
        return None
    bad = np.flatnonzero((got2 != want).any(axis=1))
    lines = [f"{label}: {bad.size} of {count} rows differ from the reference (period {D}); first rows: {bad[:10].tolist()}"]
    for m in groupings:
        lines.append(f"  rows mod {m}: {(bad[:10] % m).tolist()}")
    w = int(np.flatnonzero(got2[bad[0]] != want[bad[0]])[0])
    lines.append(f"  row {int(bad[0])}, first wrong word {w}: got {int(got2[bad[0], w]):#x}, expected {int(want[bad[0], w]):#x}")
    poison_word = poison(1, got2.dtype)[0]
    for g in bad[:10].tolist():
        same = [d for d in range(D) if d != g % D and np.array_equal(got2[g], dist2[d])]
        if same:
            near = [h for h in range(max(0, g - 64), min(count, g + 65)) if h % D == same[0]]
            kind = f"routing: the words expected for distinct input {same[0]} (carried by rows {near[:4]} nearby)"
        elif (got2[g] == poison_word).all():
            kind = "never written: every word still holds the poison value"
        else:
            nw = int((got2[g] != want[g]).sum())
            kind = f"arithmetic: the words of no distinct input ({nw} of {got2.shape[1]} words wrong)"
        lines.append(f"  row {g} (input {g % D}): {kind}")
    return "\n".join(lines)


def assert_every_row(got, want_distinct, label, groupings=()):
    """all rows of got, word for word, no tolerance, no subset"""
    msg = report(got, want_distinct, label, groupings)
    assert msg is None, msg


@contextlib.contextmanager
def options(api, opts):
    """set a dict of cufhe_amd_set_option keys; every one is back at its default on exit, whatever happened inside"""
    unknown = [k for k in opts if k not in OPTION_DEFAULTS]
    assert not unknown, f"no default recorded for {unknown}"
    try:
        for k, v in opts.items():
            api.set_option(k, v)
        yield
    finally:
        for k in opts:
            api.set_option(k, OPTION_DEFAULTS[k])


# period and largest count of each path of tests/test_gpu_positions.py (tests/test_positions.py asserts the coverage they give)
D_ORACLE = 67           # paths with a compiled oracle: about a second of reference per (set, level)
D_CHECKER = 23          # paths whose reference is a Python checker (user / multi-output gates, circuit bootstrapping): profiles/r10_every_row.md
PATHS = {
    "default": (D_ORACLE, 32768), "addressing": (D_ORACLE, 2049), "per_gate": (D_ORACLE, 32768), "lvl2": (D_ORACLE, 4096),
    "paramsets": (D_ORACLE, 4096), "trlwe": (D_ORACLE, 1031), "user_gates": (D_CHECKER, 2100), "circuit_bootstrap": (D_CHECKER, 2100),
}
