"""CPU tests of the op-id registry (cufhe_amd/csrc/op_registry.h) through tests/host/op_registry_harness.cpp: the id arithmetic of the
four ranges against the public macros, the write-once table, and the admission rule against every row of the refusal matrix recorded
on the GPU from the library as it was before the registry (tests/golden/user_op_refusals_v1.json, see its "what").  The same harness
runs once more under the address and undefined-behaviour sanitizers, as the stand-alone program it is."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_user_op_refusals as matrix  # noqa: E402

SRC = os.path.join(ROOT, "tests", "host", "op_registry_harness.cpp")
EXE = os.path.join(ROOT, "tests", "host", "op_registry_harness")
DEPS = [SRC, os.path.join(ROOT, "cufhe_amd", "csrc", "op_registry.h"), os.path.join(ROOT, "include", "cufhe_amd.h")]
CXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SET_A, SET_B = 1, 0          # indices of matrix.SET and matrix.OTHER_SET among the compiled sets (tests/test_gpu_user_op_refusals.py checks them)


def _build(exe, flags=()):
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(CXX + list(flags) + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def harness():
    return _build(EXE)


def _run(exe, *args, stdin=None):
    out = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", (out.stdout[-2000:], out.stderr[-3000:])
    return out.stdout


def _define(name):
    text = open(os.path.join(ROOT, "include", "cufhe_amd.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % re.escape(name), text).group(1))


RANGES = {"user": ("CUFHE_AMD_USER_OP_BASE", "CUFHE_AMD_MAX_USER_GATES"), "lvl2": ("CUFHE_AMD_LVL2_USER_OP_BASE", "CUFHE_AMD_LVL2_MAX_USER_GATES"),
          "ps": ("CUFHE_AMD_PS_USER_OP_BASE", "CUFHE_AMD_PS_MAX_USER_GATES"), "lookup": ("CUFHE_AMD_LOOKUP_OP_BASE", "CUFHE_AMD_MAX_LOOKUPS")}


def test_id_ranges_follow_the_public_macros(harness):
    """every id in [base - 2, end + 2) of the four ranges: contains, def and output are the arithmetic of CUFHE_AMD_*_OP_OUTPUT(base + k, j)
    = base + k + j * cap, j < 8"""
    seen = {name: [] for name in RANGES}
    for line in _run(harness, "ranges").splitlines():
        name, *v = line.split()
        seen[name].append(tuple(int(x) for x in v))
    for name, (base_macro, cap_macro) in RANGES.items():
        base, cap = _define(base_macro), _define(cap_macro)
        want = []
        for op in range(base - 2, base + 8 * cap + 2):
            inside = base <= op < base + 8 * cap
            want.append((op, 1, (op - base) % cap, (op - base) // cap) if inside else (op, 0, -1, -1))
        assert seen[name] == want, name
        ids = {base + k + j * cap for k in range(cap) for j in range(8)}
        assert ids == {op for op, inside, _, _ in seen[name] if inside}
    from cufhe_amd import api
    assert (api.USER_OP_BASE, api.LVL2_USER_OP_BASE, api.PS_USER_OP_BASE, api.LOOKUP_OP_BASE) == tuple(_define(RANGES[n][0]) for n in RANGES)
    assert (matrix.USER_BASE, matrix.LVL2_BASE, matrix.PS_BASE, matrix.LOOKUP_BASE) == tuple(_define(RANGES[n][0]) for n in RANGES)


def test_table_is_write_once_until_cleared(harness):
    assert _run(harness, "table") == "ok\n"


@pytest.fixture(scope="module")
def golden():
    return json.load(open(matrix.FIXTURE))


def test_fixture_is_the_whole_matrix(golden):
    """one row per case of the recorder, in its order; none missing, none skipped"""
    cases = matrix.cases()
    assert len(cases) == matrix.EXPECTED_ROWS == len(golden["rows"])
    assert [r[0] for r in golden["rows"]] == [c[0] for c in cases]
    assert re.search(r"commit [0-9a-f]{7,}", golden["what"])
    for name, rc, m in golden["rows"]:
        assert rc in (0, -1, -3) and 0 <= m < len(golden["messages"]), name
        assert (rc == 0) == (golden["messages"][m] == ""), name
        assert "skip" not in golden["messages"][m].lower(), name


def _requests():
    out = []
    for _, entry, route, names in matrix.cases():
        _, active, ring, level = route
        out.append(" ".join([entry, str(SET_A if active else -1), str(ring), str(level)] + [str(matrix.op_id(n)) for n in names]))
    return out


def _check_admission(exe, golden):
    texts = set(_run(exe, "texts").splitlines())
    answers = _run(exe, "admit", str(SET_A), str(SET_B), stdin="".join(r + "\n" for r in _requests())).split("\n")[:-1]
    assert len(answers) == len(golden["rows"])
    refused = 0
    for (name, rc, m), line in zip(golden["rows"], answers):
        code, text = line.split("\t")
        want = golden["messages"][m]
        if int(code):        # the registry refuses: the library said exactly this
            assert (int(code), text) == (rc, want), name
            refused += 1
        else:                # the registry lets it through: whatever the library said then, it is none of the registry's refusals
            assert want not in texts, f"{name}: the library said {want!r}, the registry admits"
    return refused, sum(1 for _, _, m in golden["rows"] if golden["messages"][m] in texts)


def test_admission_reproduces_the_recorded_refusals(harness, golden):
    """every row of the matrix in the recorder's table state: where the registry refuses, code and text are the recorded ones; where it
    admits, the recorded outcome is success or a refusal of the caller's own (an unknown built-in op, a missing operand, ...)"""
    refused, recorded = _check_admission(harness, golden)
    assert refused == recorded and refused > len(golden["rows"]) // 2


def test_harness_runs_clean_under_sanitizers(golden):
    exe = _build(EXE + "_san", SANITIZE)
    assert _run(exe, "table") == "ok\n"
    assert len(_run(exe, "ranges").splitlines()) == 4 * (8 * 64 + 4)
    _check_admission(exe, golden)


def test_null_ciphertext_comes_between_the_families_refusals():
    """cufhe_amd_enqueue_gate on the built library, no device needed: without ciphertexts an undefined default-family id says "not
    defined", an id of the ring's or of the sets' family says "null ciphertext" before anything about its path or its definition"""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "cufhe_amd", "libcufhe_amd.so"))
    lib.cufhe_amd_last_error.restype = ctypes.c_char_p
    for op, want in ((matrix.USER_BASE + 7, b"user gate op not defined"), (matrix.LVL2_BASE + 7, b"null ciphertext"), (matrix.PS_BASE + 7, b"null ciphertext"),
                     (matrix.USER_BASE + 7 + 64, b"not an output of a defined multi-output user gate (CUFHE_AMD_USER_OP_OUTPUT"), (0, b"null ciphertext")):
        assert lib.cufhe_amd_enqueue_gate(0, None, op, 0, None, None, None, None) == -1
        assert want in lib.cufhe_amd_last_error(), (op, lib.cufhe_amd_last_error())
