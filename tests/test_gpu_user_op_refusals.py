"""The refusal matrix of the user-gate op ids on the built library (tools/record_user_op_refusals.py): every id state of the three
families, on every route, through every entry point -- return code and cufhe_amd_last_error() equal, row for row, what the library
answered before the op-id registry (tests/golden/user_op_refusals_v1.json, see its "what").  All of it is host work ahead of any launch
except the few accepted cases, which run one gate on zero ciphertexts."""
import json
import os
import sys

import pytest

import oracle_lib as ol

sys.path.insert(0, os.path.join(ol.ROOT, "tools"))
import record_user_op_refusals as matrix  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(matrix.FIXTURE))
    cases = matrix.cases()
    assert len(g["rows"]) == matrix.EXPECTED_ROWS == len(cases), "the fixture is not the whole matrix"
    assert [r[0] for r in g["rows"]] == [c[0] for c in cases], "the fixture's rows are not the recorder's cases"
    assert all("skip" not in g["messages"][m].lower() for _, _, m in g["rows"])
    return g


@pytest.fixture(scope="module")
def replay(engine, oracle, keys):
    """(rc, message) of every case on the library under test; the session's engine is put back afterwards"""
    m = matrix.Matrix(engine, keys, ol.KeysLvl2(oracle, keys, seed=7), ol.Keys(ol.load_set(matrix.SET), seed=5))
    try:
        import test_op_registry
        assert (m.set, engine.api.ps_index(matrix.OTHER_SET)) == (test_op_registry.SET_A, test_op_registry.SET_B)
        yield [m.run(case) for case in matrix.cases()]
    finally:
        m.close()
        engine.SetGPUNum(1)
        engine.Initialize(keys.bk, keys.ksk)


def test_every_row_equals_the_recorded_answer(golden, replay):
    assert len(replay) == len(golden["rows"])
    differ = []
    for (name, rc, m), (got_rc, got_msg) in zip(golden["rows"], replay):
        if (got_rc, got_msg) != (rc, golden["messages"][m]):
            differ.append(f"{name}: recorded ({rc}, {golden['messages'][m]!r}), now ({got_rc}, {got_msg!r})")
    assert not differ, f"{len(differ)} rows differ:\n" + "\n".join(differ[:20])


def test_accepted_cases_are_the_recorded_ones(golden, replay):
    """the ids that run at all: a defined id of the route's own family, nothing else"""
    accepted = [name for (name, rc, _), (got_rc, _) in zip(golden["rows"], replay) if got_rc == 0]
    assert accepted == [name for name, rc, _ in golden["rows"] if rc == 0] and len(accepted) > 0
    for name in accepted:
        entry, route, ident = name.split("|")
        assert ident.split(".")[1] in ("single", "output1"), name
