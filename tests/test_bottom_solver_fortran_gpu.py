"""mg_bottom_solver / hg_bottom_solver from a Fortran host: varden_main reads them from the &PROBIN namelist of the project's own inputs file
tests/golden/inputs/inputs_bubble_3d_n40_cg (40^3 cells on one level: the multigrids coarsen to 5^3 cells / 6^3 nodes; both bottom solvers CG; visc_coef > 0, so
the viscous solves take the alpha path) and hands them to the library; three steps must give the time and dt of the Python host (varden_amd/inputs.py, what
`python -m varden_amd` runs) on the same file to 1e-12, as tests/test_fortran_gpu.py compares the two hosts on the reference's inputs."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(ROOT, "varden_amd", "fortran")
MAIN = os.path.join(FDIR, "varden_main")


def test_fortran_main_reads_the_bottom_solvers_from_the_namelist(gpu, tmp_path):
    from varden_amd import advance as adv
    from varden_amd import inputs
    if not os.path.exists(MAIN):
        if shutil.which("amdflang") is None and not os.path.exists("/opt/rocm/lib/llvm/bin/flang"):
            pytest.skip("no flang on this box and no prebuilt varden_main")
        subprocess.check_call(["make", "-s", "-C", FDIR])
    nsteps = 3
    path = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_n40_cg")
    out = subprocess.run([MAIN, path, str(nsteps)], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    frows = []
    for ln in out.stdout.splitlines():
        m = re.match(r"\s*step\s+(\d+)\s+time\s+(\S+)\s+dt\s+(\S+)\s+\|u\|max\s+(\S+)", ln)
        if m:
            frows.append((int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4))))
    assert len(frows) == nsteps, out.stdout[-3000:]
    prows, stats = [], []

    def report(G):
        prows.append((G.istep, G.time, G.dt, max(m.norm_inf() for m in G.unew)))
        stats.append((adv.last_bottom_stats("mac"), adv.last_bottom_stats("hg")))
    nl, G = inputs.run(open(path).read(), nsteps=nsteps, report=report, outdir=str(tmp_path))
    assert (G.prm.mg_bottom_solver, G.prm.hg_bottom_solver) == (2, 2)
    for f, p in zip(frows, prows):
        print("step %d: fortran time %.17g dt %.17g   python time %.17g dt %.17g" % (f[0], f[1], f[2], p[1], p[2]))
        assert f[0] == p[0]
        assert abs(f[1] - p[1]) <= 1e-12 * p[1] and abs(f[2] - p[2]) <= 1e-12 * p[2], (f, p)
        assert abs(f[3] - p[3]) <= 1e-10 * p[3], (f, p)             # (the two hosts form the initial data with their own tanh: tests/test_fortran_gpu.py)
    for mac, hg in stats:                                           # the Krylov solvers ran, and did not break down
        assert mac["iters"] > 0 and hg["iters"] > 0 and mac["breakdowns"] == 0 and hg["breakdowns"] == 0, (mac, hg)
    G.close()
