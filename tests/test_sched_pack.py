"""The stream scheduler (cufhe_amd/csrc/sched_core.h) with recorded packs -- nodes of n inputs, DeviceSched::record_pack -- on the CPU:
tests/host/sched_pack_harness.cpp records random programs of level-0 gates, packs of arity 1 .. 200 with repeated handles and positions,
readers and in-place writers of the packed TRLWEs, gates that overwrite a pack's input after the pack, re-packs into buffers that still
have readers and inputs destroyed right after the pack, against a stub device, and compares every host and device word with an
in-order interpreter -- renaming on and off, two-lane scheduling forced on and off, 1 and 3 stub devices.  It counts the hazard classes
it formed and fails a run that misses one.  The same file runs once more as a stand-alone program under AddressSanitizer and UBSan, and
three single-line mutations of a COPY of sched_core.h must each make it fail."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "sched_pack_harness.cpp")
CORE = os.path.join(ROOT, "cufhe_amd", "csrc", "sched_core.h")
HAZARDS = ("war_input_below_3", "war_input_from_3", "war_out", "waw_out", "destroyed_input")


def run(exe, seeds):
    out = subprocess.run([exe, str(seeds)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    return [json.loads(line[7:]) for line in out.stdout.splitlines() if line.startswith("RESULT ")]


def test_packs_under_every_schedule(tmp_path):
    exe = str(tmp_path / "sched_pack_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-o", exe, SRC])
    res = run(exe, 30)
    assert len(res) == 16
    assert {(r["gpus"], r["two_lane"], r["rename"], r["with_packs"]) for r in res} == {(g, t, r, p) for g in (1, 3) for t in (2, 0) for r in (1, 0) for p in (1, 0)}
    for r in res:
        if r["with_packs"]:
            assert r["packs"] > 500 and r["terms"] > 20 * r["packs"], r        # the large arities are drawn
            assert all(r[h] >= 3 for h in HAZARDS), r
    # two lanes do run on these programs without packs, so the programs with them really meet the planner (which must decline them: the
    # harness fails a flush that holds a pack and ran on lanes)
    assert sum(r["two_lane_groups"] for r in res if r["two_lane"] == 2 and r["rename"] == 1 and not r["with_packs"]) > 0


def test_the_harness_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sched_pack_harness_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    assert len(run(exe, 6)) == 16


# (what is broken, the exact source line of record_pack, its replacement)
MUTATIONS = [
    ("inputs beyond the third are not entered as readers",
     "        add_reader(pd, L);               // a later write of this input follows the pack, or takes a fresh buffer\n", "        ;\n"),
    ("the pack's level ignores the ready of inputs beyond the third",
     "for (size_t m = 0; m < n; m++) latest = std::max(latest, ins[m]->d[device_].ready);",
     "for (size_t m = 0; m < n && m < 3; m++) latest = std::max(latest, ins[m]->d[device_].ready);"),
    ("the use mark of inputs beyond the third is dropped: a destroyed input's buffer is recycled under the pack",
     "        use(pd, L);                      // a destroyed input keeps its buffer until the pack has run\n", "        ;\n"),
]


@pytest.mark.parametrize("what,old,new", MUTATIONS, ids=[m[0][:48] for m in MUTATIONS])
def test_harness_notices_a_broken_record_pack(tmp_path, what, old, new):
    """the method of test_sched_model.py: one line of a copy of sched_core.h changed, the harness must report mismatches"""
    core = open(CORE).read()
    assert core.count(old) == 1, "mutation target moved: " + old
    (tmp_path / "cufhe_amd" / "csrc").mkdir(parents=True)
    (tmp_path / "tests" / "host").mkdir(parents=True)
    (tmp_path / "cufhe_amd" / "csrc" / "sched_core.h").write_text(core.replace(old, new))
    shutil.copy(SRC, tmp_path / "tests" / "host")
    exe = str(tmp_path / "mutant")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-o", exe, str(tmp_path / "tests" / "host" / "sched_pack_harness.cpp")])
    out = subprocess.run([exe, "30"], capture_output=True, text=True, timeout=600)
    assert out.returncode != 0 and "FAIL" in out.stdout, "the harness passed a scheduler in which " + what
    assert "differ from the in-order result" in out.stderr, out.stderr[-2000:]
