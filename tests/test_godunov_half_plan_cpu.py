"""the half-workgroup grid of the fused mkflux + update march without a GPU: god_grid_half, god_chunks_slots, god_half_fits and the half argument of
god_mk_form in varden_amd/csrc/godunov_plan.h, held by tests/cpp/godunov_half_plan_check.cpp -- once optimised, once under the address and
undefined-behaviour sanitizers"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_owners_footprints_chunks_and_forms_of_the_half_workgroups(tmp_path, flags):
    exe = str(tmp_path / "godunov_half_plan_check")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "varden_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "godunov_half_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
