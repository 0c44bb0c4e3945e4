"""The stream scheduler (cufhe_amd/csrc/sched_core.h) with recorded lookups, Spreads and table rotations, on the CPU:
tests/host/sched_lut_harness.cpp records random netlists of level-0 gates, lookup groups with a level-2 third operand (what
cufhe_amd_enqueue_lookup records) and kind-2 writers of those level-2 buffers against a stub device, and checks the in-order words,
one rotation per evaluation and that a writer of a table never shares a level with a reader of its old value -- renaming on and off,
two-lane scheduling forced on and off.  The same file runs once more as a stand-alone program under AddressSanitizer and UBSan."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "sched_lut_harness.cpp")


def run(exe, seeds):
    out = subprocess.run([exe, str(seeds)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    return [json.loads(line[7:]) for line in out.stdout.splitlines() if line.startswith("RESULT ")]


def test_lookups_and_table_writers_under_every_schedule(tmp_path):
    exe = str(tmp_path / "sched_lut_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-o", exe, SRC])
    res = run(exe, 30)
    assert len(res) == 8
    for r in res:
        assert r["rotations"] == r["evaluations"] > 0, r
        if r["luts"]:
            assert r["lookups"] > 100 and r["in_place"] > 0 and r["writers"] > 50 and r["readers_behind"] > 50, r
    by = {(r["two_lane"], r["rename"], r["luts"]): r for r in res}
    # two lanes do run on these netlists without the new ops, so the programs with them really meet the planner
    assert by[(2, 1, 0)]["two_lane_groups"] > 0


def test_the_harness_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sched_lut_harness_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    res = run(exe, 6)
    assert len(res) == 8
