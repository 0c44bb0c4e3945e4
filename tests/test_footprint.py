"""CPU tests of tests/footprint.py: the arena's layout, the evidence that Arena.check can fail (a changed word planted at every kind
of place is reported with its operand, side and distance), and the coverage of include/cufhe_amd.h by the case table."""
import numpy as np
import pytest

import footprint as fp
import positions as pos

# a few operand lists: plain uint32 rows, a strided one, 64-bit elements, and an empty batch
LISTS = {
    "gate": lambda: [fp.Operand("out", np.uint32, 9, 631, "out"), fp.Operand("in0", np.uint32, 9, 631, "in"),
                     fp.Operand("in1", np.uint32, 9, 631, "in")],
    "strided": lambda: [fp.Operand("out", np.uint32, 5, 631, "out", stride=632), fp.Operand("in0", np.uint32, 5, 631, "in", stride=636)],
    "wide": lambda: [fp.Operand("tlwe2", np.uint64, 3, 2049, "in"), fp.Operand("ntt", np.float64, 3, 12288, "out"),
                     fp.Operand("trlwe", np.uint32, 3, 2048, "inout")],
    "empty": lambda: [fp.Operand("out", np.uint32, 0, 2048, "out"), fp.Operand("in", np.uint32, 0, 631, "in")],
    "small-rows": lambda: [fp.Operand("a", np.int32, 5, 7, "in"), fp.Operand("res", np.uint32, 5, 7, "out")],
}


@pytest.mark.parametrize("name", list(LISTS))
def test_layout(name):
    a = fp.Arena(name, LISTS[name]())
    assert a.base % fp.ALIGN == 0 and a.words % fp.ALIGN_WORDS == 0
    at = 0
    for o in a.operands:
        assert (a.base + 4 * o.start) % fp.ALIGN == 0 and a.view(o.name).ptr == a.base + 4 * o.start       # alignment of every operand
        assert o.start - at == o.front_guard                                                              # no overlap: in order, guards between
        assert o.front_guard >= o.row_words and o.front_guard * 4 >= 256                                  # a row and 256 bytes in front
        assert o.back_guard >= 2 * o.row_words and (o.end + o.back_guard) % fp.ALIGN_WORDS == 0           # two rows behind, to the boundary
        assert o.end - o.start == o.rows * o.stride * o.wpe and a.view(o.name).words == o.end - o.start
        at = o.end + o.back_guard
    assert at == a.words
    # every arena word is exactly one of operand word, pad word or guard word
    count = np.zeros(a.words, np.int64)
    for k, o in enumerate(a.operands):
        m = o.word_mask()
        idx = np.arange(o.start, o.end)
        count[idx] += 1
        assert np.all(a.kind[idx[m]] == 1) and np.all(a.kind[idx[~m]] == 2) and np.all(a.owner[idx] == k)
        assert int(m.sum()) == o.rows * o.row_elems * o.wpe
    assert np.all(count <= 1) and np.all((count == 0) == (a.kind == 0)) and np.all(a.owner[a.kind == 0] == -1)
    # guard and pad words carry the position-dependent pattern, outputs the poison
    pat = fp.guard_pattern(a.words)
    assert np.array_equal(a.host[a.kind != 1], pat[a.kind != 1])
    for o in a.operands:
        if o.role == "out":
            assert np.all(a.rows(a.host, o.name).view(np.uint32) == pos.POISON)


def test_guard_pattern_depends_on_the_position():
    """a guard word copied onto another guard word -- one row further, for every row size in use -- is a change"""
    pat = fp.guard_pattern(1 << 20)
    for shift in (1, 2, 64, 631, 632, 1025, 2048, 2 * 2049, 4096, 12288, 24576):
        assert not np.any(pat[shift:] == pat[:-shift]), shift
    assert np.array_equal(fp.guard_pattern(100, first=5000), fp.guard_pattern(6000)[5000:5100])


def _strided():
    a = fp.Arena("planted", [fp.Operand("in0", np.uint32, 5, 631, "in", stride=633), fp.Operand("out", np.uint32, 5, 631, "out", stride=633),
                             fp.Operand("acc", np.uint64, 5, 64, "out")])
    a.set("in0", np.arange(5 * 631, dtype=np.uint32).reshape(5, 631))
    a.upload()
    return a


def _flip(a, word):
    after = a.download()
    after[word] ^= 0x10
    return after


def test_only_outputs_written_is_clean():
    a = _strided()
    after = a.download()
    out, acc = a["out"], a["acc"]
    rows = after[out.start:out.end].reshape(5, 633)
    rows[:, :631] = 7
    after[acc.start:acc.end] = 9
    assert a.findings(after) == [] and a.check(after) is None
    assert np.all(a.rows(after, "out") == 7) and np.all(a.rows(after, "acc") == np.uint64(9 * (1 << 32) + 9))


def test_planted_single_words():
    a = _strided()
    out, inp, acc = a["out"], a["in0"], a["acc"]
    places = {
        "the last guard word before an output": (out.start - 1, "out", "before", -1),
        "the first guard word after it": (acc.end, "acc", "after", 0),
        "the last word of the trailing guard": (acc.end + acc.back_guard - 1, "acc", "after", (acc.back_guard - 1) // 2),
        "a pad word": (out.start + 2 * 633 + 631, "out", "pad", 2 * 633 + 631),
        "the last pad word": (out.end - 1, "out", "pad", 5 * 633 - 1),
        "the first word of an input": (inp.start, "in0", "input", 0),
        "the last word of an input": (inp.start + 4 * 633 + 630, "in0", "input", 4 * 633 + 630),
        "the first arena word": (0, "in0", "before", -inp.start),
    }
    for what, (word, operand, side, distance) in places.items():
        after = _flip(a, word)
        found = a.findings(after)
        assert len(found) == 1, what
        f = found[0]
        assert (f["operand"], f["side"], f["distance"], f["words"]) == (operand, side, distance, 1), (what, f)
        assert f["first_word"] == word and f["new"] != f["old"]
        msg = a.check(after)
        assert msg is not None and f"planted, {operand}:" in msg and "1 words changed" in msg, what
    # between two operands the nearer one is named
    gap = out.start - inp.end
    assert a.findings(_flip(a, inp.end + 1))[0]["operand"] == "in0" and a.findings(_flip(a, inp.end + gap - 2))[0]["operand"] == "out"


def test_planted_extra_row():
    """a full row written directly after the last row: one run, named as row `count`; and the row before the first one"""
    a = _strided()
    acc = a["acc"]
    after = a.download()
    after[acc.end:acc.end + 128] = 0x1234
    found = a.findings(after)
    assert len(found) == 1 and (found[0]["operand"], found[0]["side"], found[0]["distance"], found[0]["words"], found[0]["rows"]) == ("acc", "after", 0, 64, 0.0)
    assert "planted, acc: 64 words changed starting 0 words after the last row (= row `count`)" in a.check(after)
    after = a.download()
    after[acc.start - 128:acc.start] = 0x1234
    found = a.findings(after)
    assert len(found) == 1 and (found[0]["side"], found[0]["distance"], found[0]["rows"], found[0]["words"]) == ("before", -64, -1.0, 64)
    # the second row behind a strided output: a run per row (the pad words between keep their pattern)
    out = a["out"]
    after = a.download()
    after[out.end + 633:out.end + 633 + 631] = 5
    found = a.findings(after)
    assert len(found) == 1 and (found[0]["operand"], found[0]["side"], found[0]["distance"], found[0]["rows"]) == ("out", "after", 633, 1.0)
    assert "(= row `count` + 1)" in a.check(after)


def test_rows_the_call_must_not_write():
    """scattered operands: a slot of the output no item names holds the poison and must keep it"""
    a = _strided()
    a.written("out", [0, 2, 3])
    out = a["out"]
    after = a.download()
    after[out.start + 2 * 633] = 1
    assert a.check(after) is None
    after[out.start + 4 * 633 + 5] = 1
    f = a.findings(after)
    assert len(f) == 1 and (f[0]["operand"], f[0]["side"], f[0]["distance"]) == ("out", "row", 4 * 633 + 5)


def test_inout_rows_may_change_and_inputs_not():
    a = fp.Arena("alias", [fp.Operand("c", np.uint32, 5, 2048, "inout"), fp.Operand("exps", np.uint32, 5, 2048, "in")])
    a.set("c", np.ones((5, 2048), np.uint32))
    a.set("exps", np.ones((5, 2048), np.uint32))
    a.upload()
    after = a.download()
    after[a["c"].start:a["c"].end] = 3
    assert a.check(after) is None
    after[a["exps"].start + 2048] = 3
    assert "words of this input, row 1 word 0" in a.check(after)


def test_every_batch_symbol_of_the_header_has_a_case():
    symbols = fp.header_batch_symbols()
    assert len(symbols) >= 34 and "cufhe_amd_gate_list" in symbols and "cufhe_amd_ps_gate_batch_level" in symbols
    assert "cufhe_amd_trgsw_to_ntt_host" not in symbols and "cufhe_amd_gate" not in symbols
    missing = [s for s in symbols if s not in fp.CASES and s not in fp.EXCLUDED]
    assert not missing, f"batched entry points without a footprint case: {missing}"
    assert not [s for s in list(fp.CASES) + list(fp.EXCLUDED) if s not in symbols], "a case names a symbol the header lacks"
    assert not set(fp.CASES) & set(fp.EXCLUDED)
    # every _batch entry point writes caller-owned device arrays: nothing may be excluded today
    assert fp.EXCLUDED == {}
    assert all(s in fp.CASES for s in fp.OVERLONG)


def test_case_table_units_and_counts():
    """U comes from the library's named constants; the counts are 0, 1 and U + 1 (a workgroup per item: 3)"""
    assert fp.csrc_constant("kBatchWaves") == fp.csrc_constant("kBrWavesPerBlock")
    assert fp.csrc_constant("kKsMaxPerWg") == fp.csrc_constant("kKsWaves")
    for sym, case in fp.CASES.items():
        assert case.variants and len({v["id"] for v in case.variants}) == len(case.variants), sym
        for v in case.variants:
            u, counts = case.unit(v), case.counts(v)
            assert u >= 1 and {0, 1, u + 1 if u > 1 else 3} <= set(counts), (sym, v["id"], u, counts)
            assert all(k in pos.OPTION_DEFAULTS for k in v["opts"]), (sym, v["id"])
    assert [fp.CASES["cufhe_amd_keyswitch_batch"].counts(v) for v in fp.CASES["cufhe_amd_keyswitch_batch"].variants] == \
        [[0, 1, 3], [0, 1, 7], [0, 1, 17], [0, 1, 17], [0, 1, 17]]
    assert fp.CASES["cufhe_amd_pack_batch"].counts(fp.CASES["cufhe_amd_pack_batch"].variants[0]) == [0, 1, fp.csrc_constant("kPackTile") + 1]
    assert fp.CASES["cufhe_amd_blind_rotate_batch"].counts(dict(shape="batch")) == [0, 1, 9]
    assert fp.CASES["cufhe_amd_blind_rotate_batch"].counts(dict(shape="half")) == [0, 1, 5]
    assert fp.CASES["cufhe_amd_blind_rotate_batch"].counts(dict(shape="ll2")) == [0, 1, 3]


def test_spread_pairs_are_the_lut_tests():
    import ast
    import os
    tree = ast.parse(open(os.path.join(fp.ROOT, "tests", "test_gpu_lut.py")).read())
    lut = [ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "SPREADS"]
    assert lut == [fp.SPREADS]
