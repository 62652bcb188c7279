"""the one-workgroup tail cycles' LDS form without a GPU: varden_amd/csrc/tail_plan.h (which thread owns which cell or node, where the arrays sit in LDS,
which level sets are refused) held by tests/cpp/tail_plan_check.cpp -- once optimised, once under the address and undefined-behaviour sanitizers"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_owners_and_lds_layout_of_the_tail_cycles(tmp_path, flags):
    exe = str(tmp_path / "tail_plan_check")
    subprocess.check_call(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "varden_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "tail_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
