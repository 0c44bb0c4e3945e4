"""CPU tests of the launch-shape rules (cufhe_amd/csrc/launch_plan.h), printed by tests/host/launch_plan_harness.cpp: the plans
are the ones recorded from the launchers the header replaced (tests/golden/launch_plans_v1.json, see its "what"), the scheduler's
cost model gives the recorded milliseconds, and every plan -- the recorded grid and random (count, CUs, tuning) triples -- has the
structure the launchers rely on."""
import hashlib
import json
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "launch_plan_harness.cpp")
EXE = os.path.join(ROOT, "tests", "host", "launch_plan_harness")
DEPS = [SRC, os.path.join(ROOT, "cufhe_amd", "csrc", "launch_plan.h")]
CXX = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
CUS = [1, 8, 15, 16, 40, 104, 256, 304]
PKS_MAX_SLICES = (2049 + 15) // 16        # ceil(kPksIn / kPksIBlock), kernels_pks.hip.h
KS_SHAPES = [(1024, 1), (2048, 2)]        # (kn, min_slices): KsShapeDefault and every KsShapePs / KsShapeLvl2


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(CXX + ["-o", EXE, SRC])
    return EXE


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "launch_plans_v1.json")))


def _blocks(text):
    """'# head' + lines -> {head: lines joined as printed}"""
    out = {}
    for b in text.split("# ")[1:]:
        head, body = b.split("\n", 1)
        out[head] = body
    return out


@pytest.fixture(scope="module")
def dump_text(harness):
    return subprocess.run([harness, "dump"], capture_output=True, check=True, text=True, timeout=300).stdout


@pytest.fixture(scope="module")
def blocks(dump_text):
    return _blocks(dump_text)


def _query(exe, requests):
    out = subprocess.run([exe, "query"], input="".join(r + "\n" for r in requests), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-3000:]
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(requests)
    return lines


def _at(body, count):
    """the value at `count` of a block that prints "count value" where the value changes"""
    best = None
    for line in body.splitlines():
        n, v = line.split(" ", 1)
        if n.isdigit() and int(n) <= count:
            best = v
    return best


def _grid(cus):
    return list(range(17 * cus + 10)) + ([4600] if 17 * cus + 9 < 4600 else []) + [32768, 40960]


def _expand(points, counts):
    """[[count, value], ...] change points -> the value at every count of `counts`"""
    out, i, cur = [], 0, None
    for n in counts:
        while i < len(points) and points[i][0] <= n:
            cur = points[i][1]
            i += 1
        out.append(cur)
    return out


def _segments(text):
    """'B 0 2048 8 | P 2048 512' -> [(kernel, first, count, active)]"""
    out = []
    for s in text.split(" | ") if text else []:
        f = s.split(" ")
        out.append((f[0], int(f[1]), int(f[2]), int(f[3]) if len(f) > 3 else 0))
    return out


def _check_br(count, text):
    segs = _segments(text)
    assert len(segs) <= 3 and (count > 0 or not segs), (count, text)
    at = 0
    for kernel, first, n, active in segs:
        assert kernel in "BLP" and first == at and n > 0, (count, text)
        assert active in (4, 8) if kernel == "B" else active == 0, (count, text)
        at += n
    assert at == count, (count, text)


def _check_ks(text, min_slices):
    if text in ("S8", "W"):
        return
    k, per_wg, slices = text.split(" ")
    per_wg, slices = int(per_wg), int(slices)
    assert k == "T" and 1 <= per_wg <= 16 and min_slices <= slices <= 64 and slices & (slices - 1) == 0, text


def _check_pks(count, text):
    tiles, slices = (int(v) for v in text.split(" "))
    assert tiles == (count + 63) // 64 and 1 <= slices <= PKS_MAX_SLICES, (count, text)


def test_same_plans_as_the_recorded_ones(blocks, golden):
    """Every (rule, CU count, tuning) block of the grid prints what the launchers this header replaced launched."""
    hashed = {h: hashlib.sha256(b.encode()).hexdigest() for h, b in blocks.items() if not h.startswith(("ms ", "lane "))}
    assert sorted(hashed) == sorted(golden["sha256"]) and len(hashed) == 8 * (11 + 4 * 2 * 12 + 3 * 3 + 3 + 1)
    assert [h for h in hashed if hashed[h] != golden["sha256"][h]] == []


def test_written_out_plans(blocks, golden):
    """The plans a reader can check against DESIGN.md section 5 and the comment tables of launch_plan.h, line by line."""
    for head, lines in golden["written_out"].items():
        body = blocks[head]
        for count, want in lines.items():
            if head.startswith("br "):
                assert "\n%s: %s\n" % (count, want) in "\n" + body, (head, count)
            else:
                assert _at(body, int(count)) == want, (head, count)
    # "kn = 1024 -- 4096 ciphertexts: 256 workgroups x 1024 steps; 3072: 768 x 256 (three rounds); 2048: 256 x 512; 256: 256 x 64"
    ks = golden["written_out"]["ks path=default kn=1024 min=1 cus=256 split=-1 wg=-1 per_wg=-1 slices=-1"]
    for count, shape in ((4096, (256, 1024)), (3072, (768, 256)), (2048, (256, 512)), (256, (256, 64))):
        _, per_wg, slices = ks[str(count)].split(" ")
        assert (-(-count // int(per_wg)) * int(slices), 1024 // int(slices)) == shape
    br = golden["written_out"]["br cus=256 ll=-1 ll2=-1 half=-1 tail=1 shape=0"]
    assert sorted(int(c) for c in br) == [300, 600, 1300, 1536, 2049, 2700, 3500, 4096, 4600]


def test_cost_model_gives_the_recorded_milliseconds(blocks, golden):
    """blind_rotate_ms sums over the plan's segments what HipBackend::launch_ms computed by its own copy of the rules: sums of at
    most four terms below 1000 ms, where an ulp is about 1e-13 -- so 1e-9 admits another order of the additions and no other constant."""
    for cus in CUS:
        counts = _grid(cus)
        want = _expand(golden["ms"][str(cus)], counts)
        got = _expand([[int(n), v] for n, v in (l.split(" ") for l in blocks["ms cus=%d" % cus].splitlines())], counts)
        assert None not in want and None not in got
        worst = max(abs(float(a) - float(b)) for a, b in zip(want, got))
        assert worst <= 1e-9, (cus, worst)
        assert float(want[0]) == 0.0 and all(float(v) > 0 for v in want[1:])


def test_lane_model_is_the_recorded_one(blocks, golden):
    for cus in CUS:
        assert blocks["lane cus=%d" % cus].splitlines() == golden["lane"][str(cus)]
    assert golden["lane"]["15"][0] == "model none" and golden["lane"]["16"][0].startswith("model 16 64 ")


def test_structure_of_the_recorded_grid(blocks):
    """Segments are non-empty, in order and tile [0, count); at most three; the batch kernel runs 4 or 8 rotations per workgroup;
    key-switch and private-key-switch shapes stay inside what their kernels take."""
    seen = 0
    for head, body in blocks.items():
        rule = head.split(" ")[0]
        for line in body.splitlines():
            if rule == "br":
                count, text = line.split(":", 1)
                _check_br(int(count), text[1:])
            elif rule == "ks" and line != "0 -":
                _check_ks(line.split(" ", 1)[1], int(head.split("min=")[1].split(" ")[0]))
            elif rule == "pks" and line != "0 -":
                _check_pks(int(line.split(" ")[0]), line.split(" ", 1)[1])
            seen += 1
    assert seen > 100000


def _random_requests():
    rng = random.Random(20251018)
    big = 1 << 30
    reqs = []
    for _ in range(2000):
        count, cus = rng.choice([0, 1, rng.randrange(70001), rng.randrange(70001)]), rng.choice([0, 1, rng.randrange(513), rng.randrange(513)])
        thr = lambda: rng.choice([-1, -1, 0, big, rng.randrange(70001)])     # noqa: E731
        kn, min_slices = rng.choice(KS_SHAPES)
        reqs.append(("br", count, min_slices, "br %d %d %d %d %d %d %d" % (count, cus, thr(), thr(), thr(), rng.choice([0, 1, 1]), rng.choice([0, 0, 0, 1, 2, 3]))))
        reqs.append(("ks", count, min_slices, "ks %d %d %d %d %d %d %d %d %d %d" % (
            count, cus, kn, min_slices, rng.randrange(2), rng.randrange(2), thr(), thr(), rng.choice([-1, -1] + list(range(1, 17))),
            rng.choice([-1, -1, 1, 2, 4, 8, 16, 32, 64]))))
        reqs.append(("pks", count, min_slices, "pks %d %d" % (count, cus)))
        reqs.append(("other", count, min_slices, "ps %d %d %d %d %d" % (count, cus, rng.choice([1, 2]), rng.choice([9, 10]), thr())))
        reqs.append(("other", count, min_slices, "lvl2 %d %d %d" % (count, cus, rng.choice([-1, 0, 1]))))
        reqs.append(("other", count, min_slices, "ms %d %d" % (count, cus)))
        reqs.append(("other", count, min_slices, "lane %d %d" % (count, cus)))
    return reqs


def _check_answers(reqs, answers):
    for (rule, count, min_slices, req), text in zip(reqs, answers):
        if rule == "br":
            _check_br(count, text)
        elif rule == "ks":
            _check_ks(text, min_slices)
        elif rule == "pks":
            _check_pks(count, text)
        else:
            assert text, req


def test_structure_of_random_plans(harness):
    """2000 random (count <= 70000, CUs <= 512, tuning) triples, a quarter of them with no CU count known (cus = 0)."""
    reqs = _random_requests()
    assert sum(r[3].split(" ")[2] == "0" for r in reqs) > 2000
    _check_answers(reqs, _query(harness, [r[3] for r in reqs]))


def test_sanitizers(tmp_path, harness, dump_text):
    """The same program under AddressSanitizer + UBSan, as its own process: the same text, and no rule divides by zero or overflows
    with no CU count known (cus = 0) at any count of the random triples."""
    exe = str(tmp_path / "launch_plan_harness_asan")
    subprocess.check_call(CXX + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    out = subprocess.run([exe, "dump"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-3000:]
    assert out.stdout == dump_text
    reqs = _random_requests()
    reqs += [("br", n, 1, "br %d 0 -1 -1 -1 1 0" % n) for n in (0, 1, 7, 8, 9, 4096)]
    reqs += [("ks", n, 2, "ks %d 0 2048 2 %d 1 -1 -1 -1 -1" % (n, split8)) for n in (0, 1, 300, 4096) for split8 in (0, 1)]
    reqs += [("pks", n, 1, "pks %d 0" % n) for n in (0, 1, 64, 65, 40960)]
    answers = _query(exe, [r[3] for r in reqs])
    _check_answers(reqs, answers)
    assert answers == _query(harness, [r[3] for r in reqs])
