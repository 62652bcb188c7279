"""The refinement criteria through the Fortran main: varden_main reads tag_field / tag_comp / tag_gt / tag_lt from &PROBIN and tags with make_new_grids_by at both of its
call sites (initial grids, regrid) -- on the project's adaptive vortex tube it prints what varden_amd/inputs.py computes from the same file."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "varden_amd", "fortran")
MAIN = os.path.join(FDIR, "varden_main")


def test_fortran_main_refines_the_vortex_tube_like_the_python_mirror(gpu, tmp_path):
    """the pattern of tests/test_fortran_gpu.py::test_fortran_main_runs_the_regression_inputs_like_the_python_mirror on inputs_vortextube_3d_amr: the same boxes on
    every level after every step, time and dt to 1e-12 (the two hosts form the initial data with their own tanh / exp), two regrids, and a refined level at all"""
    from varden_amd import inputs
    if not os.path.exists(MAIN):
        if shutil.which("amdflang") is None and not os.path.exists("/opt/rocm/lib/llvm/bin/flang"):
            pytest.skip("no flang on this box and no prebuilt varden_main")
        subprocess.check_call(["make", "-s", "-C", FDIR])
    path = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_vortextube_3d_amr")
    out = subprocess.run([MAIN, path], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    frows = []
    for ln in out.stdout.splitlines():
        m = re.match(r"\s*step\s+(\d+)\s+time\s+(\S+)\s+dt\s+(\S+)\s+\|u\|max\s+(\S+)\s+levels\s+(\d+)\s+boxes\s+(.*)", ln)
        if m:
            frows.append((int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4)), int(m.group(5)), [int(x) for x in m.group(6).split()]))
    assert len(frows) == 4, out.stdout[-3000:]
    regrids = int(re.search(r"regrids:\s+(\d+)", out.stdout).group(1))
    prows = []

    def report(G):
        prows.append((G.istep, G.time, G.dt, max(m.norm_inf() for m in G.unew), G.nlev, [len(b) for b in G.boxes]))
    nl, G = inputs.run(open(path).read(), report=report, outdir=str(tmp_path))
    assert regrids == G.nregrids == 2, (regrids, G.nregrids)
    for f, p in zip(frows, prows):
        print(f, p)
        assert f[0] == p[0] and f[4] == p[4] == 2 and f[5][:p[4]] == p[5], (f, p)
        assert abs(f[1] - p[1]) <= 1e-12 * p[1] and abs(f[2] - p[2]) <= 1e-12 * p[2] and abs(f[3] - p[3]) <= 1e-10 * p[3], (f, p)
    G.close()
