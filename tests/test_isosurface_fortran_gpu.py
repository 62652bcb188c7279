"""The isosurface files from the Fortran host: varden_main (varden_amd/fortran/varden_main.f90) and varden_amd/inputs.py: run are two thin hosts over one C-ABI and
write the same files for the same input with iso_int set, byte for byte; without the key varden_main writes no such file and prints what it printed.

The comparison starts both hosts from ONE checkpoint (restart = 2), as tests/test_profiles_fortran_gpu.py does: a fresh start would hand the library two initial
states that differ in the last bit, because each host forms tanh / exp of initdata with its own mathematical library."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "varden_amd", "fortran", "varden_main")
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_n32_iso")      # two levels, regrid every second step, iso_int = 2, diag_int = 1


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
    from varden_amd import advance as adv
    from varden_amd import inputs
    start, py, fo = tmp_path / "start", tmp_path / "py", tmp_path / "fo"
    for d in (start, py, fo):
        d.mkdir()
    # the common starting point: the Python host's checkpoint after two steps
    nl, G = inputs.run(variant(max_step=2, chk_int=2, iso_int=0, diag_int=0), report=None, outdir=str(start))
    G.close()
    for d in (py, fo):
        shutil.copytree(str(start / "chk00002"), str(d / "chk00002"))
    # the density every step, then a velocity component under another name
    for kw, base, steps in ((dict(iso_int=1), "iso", (2, 3, 4)), (dict(iso_int=2, iso_field="'velocity'", iso_comp=3, iso_value="-0.001d0", iso_base_name="'w'"), "w", (2, 4))):
        text = variant(max_step=4, chk_int=0, restart=2, diag_int=0, **kw)
        nl, G = inputs.run(text, report=None, outdir=str(py))
        G.close()
        _main(text, str(fo))
        names = ["%s.dat" % base] + ["%s%05d.ply" % (base, s) for s in steps]
        for d in (py, fo):
            assert sorted(f for f in os.listdir(str(d)) if re.fullmatch(r"%s(\.dat|\d{5}\.ply)" % base, f)) == names, os.listdir(str(d))
        for f in names:
            a, b = open(str(py / f), "rb").read(), open(str(fo / f), "rb").read()
            assert a == b, "%s: inputs.run wrote %d bytes, varden_main %d\n%r\n%r" % (f, len(a), len(b), a[:400], b[:400])
        assert open(str(py / names[0])).read().count("\n") == 1 + len(steps)
        for f in names[1:]:
            assert adv.read_iso(str(fo / f))["tri"].shape[0] > 0, f


def test_without_the_key_no_file_and_the_same_stdout(gpu, tmp_path):
    off, on = tmp_path / "off", tmp_path / "on"
    off.mkdir(); on.mkdir()
    out_off = _main(variant(max_step=2, iso_int=0, diag_int=0), str(off))
    out_on = _main(variant(max_step=2, iso_int=2, diag_int=0), str(on))
    assert sorted(os.listdir(str(off))) == ["inputs"], os.listdir(str(off))
    assert sorted(os.listdir(str(on))) == ["inputs", "iso.dat", "iso00000.ply", "iso00002.ply"]
    assert out_off == out_on and len(re.findall(r"(?m)^\s*step\s+\d+\s+time", out_off)) == 2
