"""the tiles of the nodal multigrid's LDS-tiled levels without a GPU: varden_amd/csrc/nd_lds_plan.h (who owns which fine and coarse node, the working regions
inside the LDS boxes, the extents that are refused) held by tests/cpp/nd_lds_plan_check.cpp"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tiles_of_the_nodal_lds_levels(tmp_path):
    exe = str(tmp_path / "nd_lds_plan_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "varden_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "nd_lds_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
