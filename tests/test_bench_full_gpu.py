"""bench.py without and with --full: a plain run times the steps and prints the line, nothing else; --full adds the roofline probe and the
CPU baseline, whose parity with the oracle still fails the run when it is out of tolerance."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_line(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--box", "32"] + args,
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    js = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(js) == 1, out.stdout
    return json.loads(js[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_only_and_full_adds_the_other_legs(gpu):
    plain = bench_line([])
    assert plain["full"] is False and plain["steps"] == 2 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["roofline"] is None and plain["cpu_baseline"] is None and plain["extra_workloads"] == []
    full = bench_line(["--full", "--cpu-box", "32", "--cpu-steps", "1", "--no-calib"])
    assert full["full"] is True and full["steps"] == 2 and full["ms_per_step"] > 0
    assert full["roofline"]["avg_launch_ms"] > 0 and full["roofline"]["achieved"] > 0
    parity = full["cpu_baseline"]["parity"]
    assert parity["steps_compared"] == 1 and parity["cycles_equal"] and parity["max_rel_u"] <= 1e-9
    assert full["config"]["cells"] == plain["config"]["cells"] == 32 ** 3
    assert full["config"]["vcycles_per_step"] == plain["config"]["vcycles_per_step"]
