"""The profile files from the Fortran host: varden_main (varden_amd/fortran/varden_main.f90) and varden_amd/inputs.py: run are two thin hosts over one C-ABI and
write the same files for the same input with prof_int set, byte for byte; without the key varden_main writes no such file and prints what it printed.

The comparison starts both hosts from ONE checkpoint (restart = 2), as tests/test_diagnostics_fortran_gpu.py does: a fresh start would hand the library two initial
states that differ in the last bit, because each host forms tanh / exp of initdata with its own mathematical library."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "varden_amd", "fortran", "varden_main")
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_n32_prof")      # two levels, regrid every second step, prof_int = 2, diag_int = 1


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


def test_both_hosts_write_the_same_files(gpu, tmp_path):
    from varden_amd import inputs
    start, py, fo = tmp_path / "start", tmp_path / "py", tmp_path / "fo"
    for d in (start, py, fo):
        d.mkdir()
    # the common starting point: the Python host's checkpoint after two steps
    nl, G = inputs.run(variant(max_step=2, chk_int=2, prof_int=0, diag_int=0), report=None, outdir=str(start))
    G.close()
    for d in (py, fo):
        shutil.copytree(str(start / "chk00002"), str(d / "chk00002"))
    # along z (the default) every step, then along x under another name
    for kw, names in ((dict(prof_int=1), ["prof00002", "prof00003", "prof00004"]), (dict(prof_int=2, prof_axis=1, prof_base_name="'px'"), ["px00002", "px00004"])):
        text = variant(max_step=4, chk_int=0, restart=2, diag_int=0, **kw)
        nl, G = inputs.run(text, report=None, outdir=str(py))
        G.close()
        _main(text, str(fo))
        for d in (py, fo):
            assert sorted(f for f in os.listdir(str(d)) if f.startswith(names[0][:2]) and not f.startswith("chk")) == names, os.listdir(str(d))
        for f in names:
            a, b = open(str(py / f), "rb").read(), open(str(fo / f), "rb").read()
            assert a.count(b"\n") == 7 + 64 and a.split(b"\n")[2] == (b"# axis 1" if f.startswith("px") else b"# axis 3"), a[:300]
            assert a == b, "%s\ninputs.run:\n%s\nvarden_main:\n%s" % (f, a[:3000].decode(), b[:3000].decode())


def test_without_the_key_no_file_and_the_same_stdout(gpu, tmp_path):
    off, on = tmp_path / "off", tmp_path / "on"
    off.mkdir(); on.mkdir()
    out_off = _main(variant(max_step=2, prof_int=0, diag_int=0), str(off))
    out_on = _main(variant(max_step=2, prof_int=2, diag_int=0), str(on))
    assert sorted(os.listdir(str(off))) == ["inputs"], os.listdir(str(off))
    assert sorted(os.listdir(str(on))) == ["inputs", "prof00000", "prof00002"]
    assert out_off == out_on and len(re.findall(r"(?m)^\s*step\s+\d+\s+time", out_off)) == 2
