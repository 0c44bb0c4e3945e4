"""CPU tests of the recorded lookups, Spreads and table rotations ("Recorded forms"): the library exports
the four entry points and header, bindings and library agree on them; the refusals that need no device; the op-id ranges overlap no
other range (a g++ compile of static_asserts over the header's macros); the model tests/lookup_program_model.py is lut_checker on the
same words for the identity definition; its program generator plants every hazard class; and the end-to-end case of
tests/test_gpu_recorded_lut.py decrypts right on the checker alone, for the committed seed."""
import ctypes
import os
import re
import subprocess

import numpy as np

import lookup_program_model as lm
import lut_checker as lc
import oracle_lib as ol

n, N = ol.n, ol.N
NEW_SYMBOLS = ("cufhe_amd_define_lookup", "cufhe_amd_enqueue_lookup", "cufhe_amd_enqueue_spread", "cufhe_amd_enqueue_lut_rotate")
HEADER = os.path.join(ol.ROOT, "include", "cufhe_amd.h")


def test_library_exports_the_new_entry_points():
    import cufhe_amd._lib as _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto, name
        # the prototype's parameter count is the binding's
        assert len(re.sub(r"/\*.*?\*/", "", proto.group(1)).split(",")) == len(_lib.SIGNATURES[name][1]), name
    import cufhe_amd.api as api
    for name in ("DefineLookup", "Lookup", "gLookup", "gSpread", "gLutRotate"):
        assert callable(getattr(api, name))
    macros = dict(re.findall(r"#define (CUFHE_AMD_(?:LOOKUP_OP_BASE|MAX_LOOKUPS)) (\d+)", header))
    assert int(macros["CUFHE_AMD_LOOKUP_OP_BASE"]) == api.LOOKUP_OP_BASE and int(macros["CUFHE_AMD_MAX_LOOKUPS"]) == api.MAX_LOOKUPS


def test_refusals_that_need_no_device_work():
    import cufhe_amd._lib as _lib
    lib = _lib.lib
    fake, fake2 = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 28)      # never dereferenced: every call is refused before that
    op = ctypes.c_int(-1)

    def refused(rc, *words):
        msg = lib.cufhe_amd_last_error()
        assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)

    dl = lib.cufhe_amd_define_lookup
    one = (ctypes.c_int32 * 2)(1, 0)
    refused(dl(None, 0, 1, ctypes.byref(op)), b"null")
    refused(dl(one, 0, 1, None), b"null")
    refused(dl((ctypes.c_int32 * 2)(0, 1), 0, 1, ctypes.byref(op)), b"c0")
    for bad in (0, 3, 5, 16, -1):
        refused(dl(one, 0, bad, ctypes.byref(op)), b"nout")
    # well-formed, but no keys on this machine: -3, after the argument checks
    assert dl(one, 0, 1, ctypes.byref(op)) == -3 and b"Initialize" in lib.cufhe_amd_last_error()
    assert op.value == -1
    # no definition exists, so every id is refused before any handle is looked at
    outs = (ctypes.c_void_p * 1)(fake)
    for bad in (0, 16384, 16384 + 64, 16383, 16384 + 512):
        refused(lib.cufhe_amd_enqueue_lookup(0, None, bad, 0, 1, outs, fake2, fake, None), b"defined")
    sp = lib.cufhe_amd_enqueue_spread
    refused(sp(0, None, 0, None, fake, 1, 4), b"null")
    refused(sp(0, None, 0, fake, None, 1, 4), b"null")
    refused(sp(0, None, 0, fake, fake, 1, 4), b"must not be in")
    for stride, reps in ((0, 1), (-1, 4), (1, 0), (4, -1), (3, 4), (4, 3), (1, 2 * N), (2 * N, 1), (2, N), (64, 32), (1 << 20, 1 << 20)):
        refused(sp(0, None, 0, fake, fake2, stride, reps), b"powers of two")
    rt = lib.cufhe_amd_enqueue_lut_rotate
    refused(rt(0, None, 0, 1, None, fake2, fake), b"null")
    refused(rt(0, None, 0, 1, fake, None, fake2), b"null")
    refused(rt(0, None, 0, 1, fake, fake2, None), b"null")
    refused(rt(0, None, 0, 1, fake, fake, fake2), b"must not be table")
    for bad in (0, 3, 16):
        refused(rt(0, None, 0, bad, fake, fake2, ctypes.c_void_p(1 << 24)), b"nout")


RANGES = """
#include "cufhe_amd.h"
constexpr bool apart(int a0, int a1, int b0, int b1) { return a1 < b0 || b1 < a0; }      /* closed ranges */
constexpr int kLookupLo = CUFHE_AMD_LOOKUP_OP_BASE, kLookupHi = CUFHE_AMD_LOOKUP_OP_OUTPUT(CUFHE_AMD_LOOKUP_OP_BASE + CUFHE_AMD_MAX_LOOKUPS - 1, 7);
constexpr int kSpreadLo = CUFHE_AMD_TL_SPREAD(0, 0), kSpreadHi = CUFHE_AMD_TL_SPREAD(10, 0);
constexpr int kRotLo = CUFHE_AMD_TL_LUT_ROTATE(0), kRotHi = CUFHE_AMD_TL_LUT_ROTATE(3);
constexpr bool clear_of_existing(int lo, int hi)
{
    return apart(lo, hi, 0, CUFHE_AMD_NUM_OPS - 1) && apart(lo, hi, CUFHE_AMD_TL_BOOTSTRAP, CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP) &&
           apart(lo, hi, 1000, 1512) && apart(lo, hi, 2048, 3071) && apart(lo, hi, 4096, 6143) && apart(lo, hi, 8192, 8703) &&
           apart(lo, hi, 12288, 12799);
}
static_assert(clear_of_existing(kLookupLo, kLookupHi), "lookup ids");
static_assert(clear_of_existing(kSpreadLo, kSpreadHi), "Spread ids");
static_assert(clear_of_existing(kRotLo, kRotHi), "table-rotation ids");
static_assert(apart(kLookupLo, kLookupHi, kSpreadLo, kSpreadHi) && apart(kLookupLo, kLookupHi, kRotLo, kRotHi) && apart(kSpreadLo, kSpreadHi, kRotLo, kRotHi), "one another");
/* every (a, b) with a + b <= 10 lies inside the Spread range and names one pair only: b < 16 */
static_assert(CUFHE_AMD_TL_SPREAD(0, 10) < CUFHE_AMD_TL_SPREAD(1, 0) && CUFHE_AMD_TL_SPREAD(0, 10) <= kSpreadHi, "Spread ids are unique");
static_assert(CUFHE_AMD_USER_OP_BASE == 1000 && CUFHE_AMD_TL_SEIKS_AT(0) == 2048 && CUFHE_AMD_TL_CMUX_ROTATE(0) == 4096 &&
              CUFHE_AMD_LVL2_USER_OP_BASE == 8192 && CUFHE_AMD_PS_USER_OP_BASE == 12288, "the existing ranges are where this file says");
int main() { return 0; }
"""


def test_op_id_ranges_overlap_no_existing_range(tmp_path):
    src = tmp_path / "ranges.cpp"
    src.write_text(RANGES)
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ol.ROOT, "include"), str(src)])
    # and the check can fail: the same file with the lookup base moved into the parameter sets' range does not compile
    bad = tmp_path / "bad.cpp"
    bad.write_text(RANGES.replace('#include "cufhe_amd.h"', '#include "cufhe_amd.h"\n#undef CUFHE_AMD_LOOKUP_OP_BASE\n#define CUFHE_AMD_LOOKUP_OP_BASE 12000'))
    assert subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ol.ROOT, "include"), str(bad)],
                          capture_output=True).returncode != 0


def test_identity_definition_is_the_batch_lookup(keys):
    """coefficients (1, 0), offset 0: the address is in0, word for word, so the model is lut_checker.lut_lookup by construction; and a
    two-operand address is the sum the rotation descriptor forms (user_gate_checker.lincomb)"""
    import user_gate_checker as uc
    rng = np.random.default_rng(2200)
    x = rng.integers(0, 1 << 32, size=(2, n + 1), dtype=np.uint64).astype(np.uint32)
    table = rng.integers(0, 1 << 32, size=2 * N, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(lm.address(1, 0, 0, x[0]), x[0])
    assert np.array_equal(lm.lookup(keys, (1, 0, 0, 2), table, x[0]), lc.lut_lookup(keys, x[0], table, 2))
    for c0, c1, off in ((1, 1, 0x2468ACE1), (-1, 1, 0x9ABCDEF0), (3, -2, 7)):
        assert np.array_equal(lm.address(c0, c1, off, x[0], x[1]), uc.lincomb((c0, c1, 0), [x[0], x[1]], off))


def test_generator_plants_every_hazard():
    for seed in range(2400, 2420):
        init_c, init_t, prog = lm.generate(seed, 40)
        assert 36 <= len(prog) <= 44
        h = lm.hazards(prog)
        assert all(h[k] >= 1 for k in lm.HAZARDS), (seed, h)
        kinds = {op["kind"] for op in prog}
        assert {"nand", "lookup", "spread"} <= kinds
        for op in prog:
            if op["kind"] == "lookup":
                nout = lm.DEFS[op["d"]][3]
                slots = [s for s, _ in op["outs"]]
                assert len(set(slots)) == len(slots) and all(0 <= j < nout for _, j in op["outs"])
                if nout > 1:
                    assert op["a"] not in slots and op["b"] not in slots
    nouts = {lm.DEFS[op["d"]][3] for s in range(2400, 2420) for op in lm.generate(s, 40)[2] if op["kind"] == "lookup"}
    assert nouts == {1, 2, 8}


def test_end_to_end_case_decrypts_on_the_checker(keys):
    """the committed case of test_gpu_recorded_lut.py::test_end_to_end_under_genuine_keys on the checker alone: every one of the p = 4
    addresses reads its entry, and the two-operand address 1/8 + 2/8 reads entry 3 -- zero errors.  The GPU case compares words with
    these, so it inherits the decryption."""
    table_words, addrs, v = lm.worked_example_inputs(keys)
    assert set(v) == {0, 1}
    table = lm.spread(table_words, 1, N // 4)
    outs = lc.on_threads(lambda m: lm.lookup(keys, (1, 0, 0, 1), table, addrs[m])[0], 4)
    errors = sum(int(keys.decrypt(outs[m], 0)[0]) != int(v[m]) for m in range(4))
    assert errors == 0, ([int(keys.decrypt(o, 0)[0]) for o in outs], list(v))
    fifth = lm.lookup(keys, (1, 1, 0, 1), table, addrs[1], addrs[2])[0]
    assert int(keys.decrypt(fifth, 0)[0]) == int(v[3])
