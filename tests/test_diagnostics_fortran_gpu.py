"""The diagnostics file from the Fortran host: varden_main (varden_amd/fortran/varden_main.f90) and varden_amd/inputs.py: run are two thin hosts over one C-ABI and
write the same file for the same input with diag_int = 1, character for character; without the key varden_main writes no such file and prints what it printed.

The byte-for-byte comparison starts both hosts from ONE checkpoint (restart = 2): a fresh start would hand the library two initial states that differ in the last
bit, because each host forms tanh / exp of initdata with its own mathematical library (tests/test_fortran_gpu.py holds fresh runs to 1e-12 for that reason).  The
fresh runs are compared here too, figure by figure, with that allowance."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "varden_amd", "fortran", "varden_main")
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_vortextube_3d_amr")      # two levels, regrid every second step


def variant(**kw):
    t = open(INPUTS).read()
    for k, v in kw.items():
        t, n = re.subn(r"(?mi)^(\s*%s\s*=\s*)[^!\n]*" % k, lambda m: m.group(1) + str(v) + " ", t)
        if n == 0:
            t = re.sub(r"(?m)^\s*/\s*$", " %s = %s\n/" % (k, v), t, count=1)
    return t


def _main(text, cwd):
    if not os.path.exists(MAIN):
        if shutil.which("amdflang") is None and not os.path.exists("/opt/rocm/lib/llvm/bin/flang"):
            pytest.skip("no flang on this box and no prebuilt varden_main")
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(MAIN)])
    with open(os.path.join(cwd, "inputs"), "w") as f:
        f.write(text)
    out = subprocess.run([MAIN, "inputs"], cwd=cwd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout


def test_both_hosts_write_the_same_file(gpu, tmp_path):
    from varden_amd import advance as adv
    from varden_amd import inputs
    start, py, fo = tmp_path / "start", tmp_path / "py", tmp_path / "fo"
    for d in (start, py, fo):
        d.mkdir()
    # the common starting point: the Python host's checkpoint after two steps
    nl, G = inputs.run(variant(max_step=2, chk_int=2), report=None, outdir=str(start))
    G.close()
    for d in (py, fo):
        shutil.copytree(str(start / "chk00002"), str(d / "chk00002"))
    text = variant(max_step=4, chk_int=0, restart=2, diag_int=1)
    nl, G = inputs.run(text, report=None, outdir=str(py))
    G.close()
    _main(text, str(fo))
    a, b = open(str(py / "varden_diag.out"), "rb").read(), open(str(fo / "varden_diag.out"), "rb").read()
    assert a.count(b"\n") == 4 and a.split(b"\n")[1].split()[0] == b"2", a[:400]          # the header, the starting state (step 2), steps 3 and 4
    assert a == b, "inputs.run:\n%s\nvarden_main:\n%s" % (a.decode(), b.decode())
    # fresh starts, under another file name: the same header, steps, counts and volume; the mass to 1e-10 (the hosts' own tanh and exp in initdata)
    text = variant(max_step=3, diag_int=1, diag_file_name="'fresh.out'")
    nl, G = inputs.run(text, report=None, outdir=str(py))
    G.close()
    _main(text, str(fo))
    la, lb = open(str(py / "fresh.out")).read().splitlines(), open(str(fo / "fresh.out")).read().splitlines()
    assert la[0] == lb[0] and len(la) == len(lb) == 5
    cols = ["step", "time", "dt"] + adv.diag_columns(2, 3)
    for x, y in zip(la[1:], lb[1:]):
        x, y = x.split(), y.split()
        for name in ("step", "cells", "nonfinite", "volume"):
            assert x[cols.index(name)] == y[cols.index(name)], (name, x, y)
        mx, my = float(x[cols.index("sum_s1")]), float(y[cols.index("sum_s1")])
        assert abs(mx - my) <= 1e-10 * abs(mx), (mx, my)


def test_without_the_key_no_file_and_the_same_stdout(gpu, tmp_path):
    off, on = tmp_path / "off", tmp_path / "on"
    off.mkdir(); on.mkdir()
    out_off = _main(variant(max_step=3), str(off))
    out_on = _main(variant(max_step=3, diag_int=2), str(on))
    assert sorted(os.listdir(str(off))) == ["inputs"], os.listdir(str(off))
    assert sorted(os.listdir(str(on))) == ["inputs", "varden_diag.out"]
    assert open(str(on / "varden_diag.out")).read().count("\n") == 3                        # the header, the starting state, step 2
    assert out_off == out_on and len(re.findall(r"(?m)^\s*step\s+\d+\s+time", out_off)) == 3
