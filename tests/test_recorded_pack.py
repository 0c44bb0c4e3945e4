"""CPU tests of the recorded pack (cufhe_amd_enqueue_pack, INTEGRATION.md section 12, "The recorded form"): header, bindings and library
agree on the symbol; the refusals that need no device; the op id 6912 lies in no other id range (a g++ compile of static_asserts over
the header's macros); and the model tests/pack_program_model.py is pack_checker.pack_batch on three small cases."""
import ctypes
import os
import re
import subprocess

import numpy as np

import oracle_lib as ol
import pack_checker as pk
import pack_program_model as pm

n, N = ol.n, ol.N
HEADER = os.path.join(ol.ROOT, "include", "cufhe_amd.h")
NAME = "cufhe_amd_enqueue_pack"


def test_header_bindings_and_library_agree():
    import cufhe_amd._lib as _lib
    import cufhe_amd.api as api
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(HEADER).read()
    assert hasattr(lib, NAME) and NAME in _lib.SIGNATURES
    proto = re.search(r"\bint " + NAME + r"\(([^;]*)\);", header)
    assert proto
    assert len(re.sub(r"/\*.*?\*/", "", proto.group(1)).split(",")) == len(_lib.SIGNATURES[NAME][1]) == 7
    for name in ("gPack", "Pack"):
        assert callable(getattr(api, name))
    assert int(re.search(r"#define CUFHE_AMD_TL_PACK (\d+)", header).group(1)) == api.TL_PACK == 6912
    # nothing new that tests/test_footprint.py would ask a footprint case for
    assert not NAME.endswith("_batch") and not NAME.endswith("_batch_level")
    hpp = open(os.path.join(ol.ROOT, "include", "cufhe_amd.hpp")).read()
    assert "inline void gPack(cuFHETRLWElvl1& out" in hpp and "inline void Pack(cuFHETRLWElvl1& out" in hpp


def test_refusals_that_need_no_device_work():
    import cufhe_amd._lib as _lib
    lib = _lib.lib
    call = lib.cufhe_amd_enqueue_pack

    def refused(rc, *words):
        msg = lib.cufhe_amd_last_error()
        assert rc == -1 and msg and all(w in msg for w in words), (rc, msg)

    # stand-ins for handles: the level is a handle's first member (struct cufhe_amd_ctxt, sched_core.h) and the only one these refusals
    # read; the rest of each block is zero
    def handle(level):
        buf = (ctypes.c_int32 * 1024)()
        buf[0] = level
        return buf

    trlwe, tlwe = handle(2), handle(0)
    p_trlwe, p_tlwe = ctypes.addressof(trlwe), ctypes.addressof(tlwe)
    one = (ctypes.c_void_p * 1)(p_tlwe)
    zero = (ctypes.c_int32 * 1)(0)
    refused(call(0, None, 0, None, 1, one, zero), b"null")
    refused(call(0, None, 0, p_trlwe, 1, None, zero), b"null")
    refused(call(0, None, 0, p_trlwe, 1, one, None), b"null")
    refused(call(0, None, 0, p_trlwe, 1, (ctypes.c_void_p * 1)(None), zero), b"null")
    refused(call(0, None, 0, p_trlwe, 0, one, zero), b"count_in")
    many = (ctypes.c_void_p * (N + 1))(*([p_tlwe] * (N + 1)))
    refused(call(0, None, 0, p_trlwe, N + 1, many, (ctypes.c_int32 * (N + 1))()), b"count_in")
    for bad in (-1, N):
        refused(call(0, None, 0, p_trlwe, 1, one, (ctypes.c_int32 * 1)(bad)), b"pos")
        refused(call(0, None, 0, p_trlwe, 3, (ctypes.c_void_p * 3)(p_tlwe, p_tlwe, p_tlwe), (ctypes.c_int32 * 3)(0, N - 1, bad)), b"pos")
    # wrong levels: out is no TRLWE; an input (the fourth) is no lvl0 ciphertext
    refused(call(0, None, 0, p_tlwe, 1, one, zero), b"level")
    for level in (1, 3):
        refused(call(0, None, 0, ctypes.addressof(handle(level)), 1, one, zero), b"level")
    four = (ctypes.c_void_p * 4)(p_tlwe, p_tlwe, p_tlwe, p_trlwe)
    refused(call(0, None, 1, p_trlwe, 4, four, (ctypes.c_int32 * 4)()), b"level")
    # a device that SetGPUNum does not know
    refused(call(99, None, 0, p_trlwe, 1, one, zero), b"device")


RANGES = """
#include "cufhe_amd.h"
constexpr bool apart(int a0, int a1, int b0, int b1) { return a1 < b0 || b1 < a0; }      /* closed ranges */
constexpr int kPack = CUFHE_AMD_TL_PACK;
static_assert(kPack == 6912, "the id the documents name");
static_assert(apart(kPack, kPack, 0, CUFHE_AMD_NUM_OPS - 1) && apart(kPack, kPack, CUFHE_AMD_TL_BOOTSTRAP, CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP) &&
              apart(kPack, kPack, CUFHE_AMD_USER_OP_BASE, 1512) && apart(kPack, kPack, CUFHE_AMD_TL_SEIKS_AT(0), CUFHE_AMD_TL_SEIKS_AT(1023)) &&
              apart(kPack, kPack, CUFHE_AMD_TL_CMUX_ROTATE(0), CUFHE_AMD_TL_CMUX_ROTATE(2047)) &&
              apart(kPack, kPack, CUFHE_AMD_TL_SPREAD(0, 0), CUFHE_AMD_TL_SPREAD(10, 0)) &&
              apart(kPack, kPack, CUFHE_AMD_TL_LUT_ROTATE(0), CUFHE_AMD_TL_LUT_ROTATE(3)) &&
              apart(kPack, kPack, CUFHE_AMD_LVL2_USER_OP_BASE, CUFHE_AMD_LVL2_USER_OP_BASE + 511) &&
              apart(kPack, kPack, CUFHE_AMD_PS_USER_OP_BASE, CUFHE_AMD_PS_USER_OP_BASE + 511) &&
              apart(kPack, kPack, CUFHE_AMD_LOOKUP_OP_BASE, CUFHE_AMD_LOOKUP_OP_OUTPUT(CUFHE_AMD_LOOKUP_OP_BASE + CUFHE_AMD_MAX_LOOKUPS - 1, 7)),
              "the pack's id lies in no other id range");
static_assert(CUFHE_AMD_TL_LUT_ROTATE(3) < kPack && kPack < CUFHE_AMD_LVL2_USER_OP_BASE, "between the table rotations and the lvl2 user gates");
int main() { return 0; }
"""


def test_op_id_lies_in_no_other_range(tmp_path):
    src = tmp_path / "ranges.cpp"
    src.write_text(RANGES)
    inc = "-I" + os.path.join(ol.ROOT, "include")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", inc, str(src)])
    # and the check can fail: with the id moved onto a table rotation's the same file does not compile
    bad = tmp_path / "bad.cpp"
    bad.write_text(RANGES.replace('#include "cufhe_amd.h"', '#include "cufhe_amd.h"\n#undef CUFHE_AMD_TL_PACK\n#define CUFHE_AMD_TL_PACK 6657')
                   .replace("kPack == 6912", "kPack == 6657"))
    assert subprocess.run(["g++", "-std=c++17", "-fsyntax-only", inc, str(bad)], capture_output=True).returncode != 0


def test_model_is_pack_batch_on_small_cases():
    """pack_program_model.Model.pack / run against pack_checker.pack_batch with count_out = 1 and dst all 0, under a key of random
    words cut to 8 rows of i (the formulas do not care): a single term, repeated handles and positions, and a re-pack after one of
    the inputs' slot was overwritten (issue order: the first pack keeps the old words)"""
    rows = 8
    rng = np.random.default_rng(2600)
    key = rng.integers(0, 1 << 32, size=rows * pk.T * pk.NUMBASE * pk.ROW_WORDS, dtype=np.uint64).astype(np.uint32)
    x = pk.edge_inputs(rng, 6)
    m = pm.Model(key, rows=rows)
    zeros = lambda k: np.zeros(k, np.int32)
    assert np.array_equal(m.pack([x[2]], [1023]), pk.pack_batch(key, x[2:3], zeros(1), [1023], 1, rows)[0])
    idx, pos = [0, 1, 3, 1, 5, 0], [0, 511, 7, 511, 1023, 0]      # handle 1 twice at one position, the last term repeats the first
    assert np.array_equal(m.pack([x[i] for i in idx], pos), pk.pack_batch(key, x[idx], zeros(6), pos, 1, rows)[0])
    prog = [{"kind": "pack", "tout": 0, "ins": [0, 1, 2, 3, 4], "pos": [4, 3, 2, 1, 0]},
            {"kind": "pack", "tout": 1, "ins": [4, 4], "pos": [9, 10]},
            {"kind": "pack", "tout": 0, "ins": [5], "pos": [6]}]
    c, t = m.run(list(x), [np.zeros(2 * N, np.uint32)] * 2, prog[:2])
    assert np.array_equal(t[0], pk.pack_batch(key, x[:5], zeros(5), [4, 3, 2, 1, 0], 1, rows)[0])
    assert np.array_equal(t[1], pk.pack_batch(key, x[[4, 4]], zeros(2), [9, 10], 1, rows)[0])
    c, t = m.run(list(x), [np.zeros(2 * N, np.uint32)] * 2, prog)
    assert np.array_equal(t[0], pk.pack_batch(key, x[5:6], zeros(1), [6], 1, rows)[0])      # a pack overwrites, it does not add to the old value
