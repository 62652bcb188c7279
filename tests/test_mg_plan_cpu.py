"""the multigrid hierarchy rule without a GPU: varden_amd/csrc/mg_plan.h (which levels stay distributed, which are gathered, where the boxes sit in the gather
buffers, which bottom is whole, the bottom-solver mapping) held against hand-derived shapes and the oracle's level count by tests/cpp/mg_plan_check.cpp"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hierarchy_rule_of_the_level_plan(tmp_path):
    exe = str(tmp_path / "mg_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "varden_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "mg_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
