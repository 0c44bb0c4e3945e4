"""The stream scheduler (cufhe_amd/csrc/sched_core.h) with multi-output gates, on the CPU: tests/sched_multi_output_harness.cpp records
random netlists with sibling groups (DeviceSched::record_gate_group, what cufhe_amd_enqueue_gate_multi calls) against a stub device
and checks the in-order words and one rotation per group, two-lane scheduling forced on and off, renaming on and off."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sched_multi_output_harness.cpp")


def test_sibling_groups_cost_one_rotation_under_every_schedule(tmp_path):
    exe = str(tmp_path / "sched_multi_output_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-o", exe, SRC])
    out = subprocess.run([exe, "30"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALL PASS" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    res = [json.loads(line[7:]) for line in out.stdout.splitlines() if line.startswith("RESULT ")]
    assert len(res) == 8
    for r in res:
        assert r["rotations"] == r["evaluations"] > 0, r
    by = {(r["two_lane"], r["rename"], r["groups"]): r for r in res}
    # two lanes do run on these programs without groups (so the groups' programs really exercise the planner's refusal)
    assert by[(2, 1, 0)]["two_lane_groups"] > 0
    assert by[(2, 1, 1)]["two_lane_groups"] == 0
