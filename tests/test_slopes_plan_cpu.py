"""the pair form of the slopes march without a GPU: varden_amd/csrc/slopes_plan.h (which lane owns which two cells, the full and the narrow row segments, the
rows staged in LDS, the k-chunks, the alignment rules) held by tests/cpp/slopes_plan_check.cpp -- once optimised, once under the address and
undefined-behaviour sanitizers"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_owners_alignment_and_lds_of_the_pair_form(tmp_path, flags):
    exe = str(tmp_path / "slopes_plan_check")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "varden_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "slopes_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
