"""CPU tests of the packed-ROM operations: the checker tests/packed_rom_checker.py is pinned against the
oracle and against itself before the GPU tests rely on it; the library exports the new entry points and the header's op-id ranges
are disjoint."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import packed_rom_checker as pr
import user_gate_checker as uc

N = ol.N
NEW_SYMBOLS = ("cufhe_amd_trlwe_rotate_batch", "cufhe_amd_cmux_rotate_batch", "cufhe_amd_sample_extract_index_batch",
               "cufhe_amd_sample_extract_index_keyswitch_batch", "cufhe_amd_enqueue_cmux_rotate")


def random_trlwe(rng):
    return rng.integers(0, 1 << 32, size=2 * N, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("j", [0, 1, 2, 511, 1022, 1023])
def test_the_two_forms_of_extraction_agree(oracle, j):
    """the formula in numpy and orc_sample_extract0 of X^-j c give the same N + 1 words"""
    rng = np.random.default_rng(300 + j)
    for _ in range(4):
        c = random_trlwe(rng)
        assert np.array_equal(pr.extract_formula(c, j), pr.extract_by_rotation(oracle, c, j))


def test_index_zero_is_the_oracles_extraction(oracle):
    rng = np.random.default_rng(310)
    c = random_trlwe(rng)
    want = np.zeros(N + 1, np.uint32)
    oracle.orc_sample_extract0(want, c)
    assert np.array_equal(pr.extract_formula(c, 0), want)
    assert np.array_equal(pr.extract_by_rotation(oracle, c, 0), want)


def test_rotation_has_an_inverse():
    rng = np.random.default_rng(320)
    c = random_trlwe(rng)
    assert np.array_equal(pr.rotate(c, 0), c)
    assert np.array_equal(pr.rotate(c, N), (0 - c.astype(np.uint64)).astype(np.uint32))
    for e in list(pr.EXPONENTS[1:]) + [int(x) for x in rng.integers(1, 2 * N, size=8)]:
        assert np.array_equal(pr.rotate(pr.rotate(c, e), 2 * N - e), c), e


def test_extraction_at_j_has_the_phase_of_coefficient_j(keys):
    """SE_j of a TRLWE encryption decrypts, under the lvl1 key as a TLWE, to exactly the phase of coefficient j"""
    rng = np.random.default_rng(330)
    msgs = rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32)
    c = pr.encrypt_trlwe(keys, msgs, 64.0, seed=331)
    ph = pr.trlwe_phase(keys, c)
    noise = (ph.astype(np.int64) - msgs.astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)
    assert np.abs(noise).max() < 64 * 8                        # it is an encryption of msgs
    for j in (0, 1, 2, 63, 64, 511, 1022, 1023):
        t1 = pr.extract_formula(c, j)
        assert uc.phase(keys, 1, t1)[0] == ph[j], j


def test_checker_rom_program_reads_every_word(keys):
    """the oracle composition of the recorded program decrypts to the ROM word (two addresses here; the GPU test reads all 8 against these words)"""
    table = pr.rom_table(340)
    trlwes = pr.rom_trlwes(keys, table, seed=341)
    for addr in (0, 5):
        bits = [(addr >> k) & 1 for k in range(3)]
        sels = [pr.selector(keys, bits[k], which=k) for k in range(3)]
        out = pr.rom_read(keys, trlwes, sels)
        word = sum(int(b) << i for i, b in enumerate(keys.decrypt(out, 0)))
        assert word == int(table[addr >> 2, addr & 3]), addr


def test_library_exports_the_new_entry_points():
    import cufhe_amd._lib as _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ol.ROOT, "include", "cufhe_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    for macro in ("CUFHE_AMD_TL_SEIKS_AT(j)", "CUFHE_AMD_TL_CMUX_ROTATE(e)"):
        assert macro in header
    import cufhe_amd.api as api
    assert api.TL_SEIKS_AT(0) == pr.TL_SEIKS_AT_BASE and api.TL_CMUX_ROTATE_BASE == pr.TL_CMUX_ROTATE_BASE


def test_op_id_ranges_do_not_overlap(tmp_path):
    """a C++ compile of the header: the SEIKS_AT and CMUX_ROTATE ranges lie clear of each other, of both enums and of the user gates"""
    src = tmp_path / "ranges.cpp"
    src.write_text('''
#include "cufhe_amd.h"
constexpr int kN = 1024;
constexpr int kUserLast = CUFHE_AMD_USER_OP_OUTPUT(CUFHE_AMD_USER_OP_BASE + CUFHE_AMD_MAX_USER_GATES - 1, 7);
static_assert(kUserLast == 1000 + 8 * 64 - 1, "user-gate range");
static_assert((int)CUFHE_AMD_NUM_OPS <= (int)CUFHE_AMD_TL_BOOTSTRAP && (int)CUFHE_AMD_TL_CIRCUIT_BOOTSTRAP < CUFHE_AMD_USER_OP_BASE, "enums below user gates");
static_assert(CUFHE_AMD_TL_SEIKS_AT(0) > kUserLast, "SEIKS_AT above the user gates");
static_assert(CUFHE_AMD_TL_SEIKS_AT(kN - 1) < CUFHE_AMD_TL_CMUX_ROTATE(0), "SEIKS_AT below CMUX_ROTATE");
static_assert(CUFHE_AMD_TL_SEIKS_AT(-1) > kUserLast && CUFHE_AMD_TL_SEIKS_AT(kN) < CUFHE_AMD_TL_CMUX_ROTATE(0), "out-of-range indices name no op");
static_assert(CUFHE_AMD_TL_CMUX_ROTATE(2 * kN - 1) == 6143, "CMUX_ROTATE range");
int main() { return 0; }
''')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ol.ROOT, "include"), str(src)])


def test_cpp_program_compiles():
    """tests/cpp/test_packed_rom.cpp builds against include/cufhe_amd.hpp, the library and the oracle (it runs in the GPU suite)"""
    assert os.path.exists(pr.build_cpp_program())
