"""the launch-form switches without a GPU: the reading rules of varden_amd/csrc/vdn_switches.h (tests/cpp/switches_check.cpp, built as the testing build and
as the release build reads the header) and the environment tests/children.py gives a variant's child process"""
import os
import subprocess

import pytest

from tests import children

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("define", [["-DVDN_TESTING_BUILD"], []], ids=["testing", "release"])
def test_reading_rules_of_the_switch_list(tmp_path, define):
    exe = str(tmp_path / "switches_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror"] + define + ["-I", os.path.join(ROOT, "varden_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "switches_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


def test_variant_env_drops_every_outer_switch(monkeypatch):
    for k in [k for k in os.environ if k.startswith("VDN_")]:
        monkeypatch.delenv(k)
    for k, v in (("VDN_MAC_SPLIT", "0"), ("VDN_SOMETHING_UNKNOWN", "1"), ("VDN_LIB_FLAVOUR", "testing"), ("VDN_WORKER_ORACLE", "0")):
        monkeypatch.setenv(k, v)
    vdn = lambda env: {k: v for k, v in env.items() if k.startswith("VDN_")}   # noqa: E731
    env = children.variant_env({"VDN_MAC_SPLIT_MIN": "0"})
    assert vdn(env) == {"VDN_LIB_FLAVOUR": "testing", "VDN_WORKER_ORACLE": "0", "VDN_MAC_SPLIT_MIN": "0"}
    assert {k: v for k, v in env.items() if not k.startswith("VDN_")} == {k: v for k, v in os.environ.items() if not k.startswith("VDN_")}
    assert vdn(children.variant_env({})) == {"VDN_LIB_FLAVOUR": "testing", "VDN_WORKER_ORACLE": "0"}
    # a name asked for is kept, the bench's own variables always; the variant's value wins over a kept one
    monkeypatch.setenv("VDN_BENCH_ONE_DEVICE", "1")
    assert vdn(children.variant_env({"VDN_MAC_SPLIT": "1"}, keep=("VDN_MAC_SPLIT", "VDN_SOMETHING_UNKNOWN"))) == {
        "VDN_LIB_FLAVOUR": "testing", "VDN_WORKER_ORACLE": "0", "VDN_BENCH_ONE_DEVICE": "1", "VDN_SOMETHING_UNKNOWN": "1", "VDN_MAC_SPLIT": "1"}
    assert "VDN_MAC_SPLIT" in os.environ          # (the caller's environment is left alone)
