"""The Fortran host (varden_amd/fortran/varden_main.f90) on a 2-D hierarchy: it writes the 2-D run's own dm = 2 files (fabio_ml_multifab_write_plane_d,
checkpoint_write_plane, make_vorticity_plane of varden_amd_mod.f90) on the boxes the Python host's files list, and restarts from its own checkpoint
(restart_copy_from_planes: the extrude_boxes rule restated in Fortran, fabio_ml_multifab_read_plane_d)."""
import os
import re
import shutil
import subprocess

import pytest

from tests.test_plane_io_gpu import INPUTS, variant
from tests.util import WALLS, params_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "varden_amd", "fortran", "varden_main")
STEP = re.compile(r"\s*step\s+(\d+)\s+time\s+(\S+)\s+dt\s+(\S+)\s+\|u\|max\s+(\S+)")


def _main(inputs_path, cwd):
    out = subprocess.run([MAIN, inputs_path], cwd=cwd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return {int(m.group(1)): tuple(float(m.group(i)) for i in (2, 3, 4)) for m in map(STEP.match, out.stdout.splitlines()) if m}


def test_fortran_main_writes_plane_files_and_restarts_from_them(gpu, tmp_path):
    from varden_amd import inputs, plotfile
    if not os.path.exists(MAIN):
        if shutil.which("amdflang") is None and not os.path.exists("/opt/rocm/lib/llvm/bin/flang"):
            pytest.skip("no flang on this box and no prebuilt varden_main")
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(MAIN)])
    a, b, py = tmp_path / "a", tmp_path / "b", tmp_path / "py"
    for d in (a, b, py):
        d.mkdir()
    (a / "inputs").write_text(open(INPUTS).read())
    (b / "inputs").write_text(variant(restart=2))
    rows_a = _main("inputs", str(a))
    assert sorted(rows_a) == [1, 2, 3, 4]
    assert sorted(p for p in os.listdir(str(a)) if p[:3] in ("plt", "chk")) == ["chk0000%d" % i for i in range(5)] + ["plt00000", "plt00002", "plt00004"]
    r = plotfile.read_ml_multifab(str(a / "plt00002"))
    assert r["dm"] == 2 and r["names"] == plotfile.plot_names(2, 2) and all(f.shape[2:] == (1, 8) for L in r["levels"] for f in L["fabs"])
    assert min(f[..., 5].min() for L in r["levels"] for f in L["fabs"]) < 0 < max(f[..., 5].max() for L in r["levels"] for f in L["fabs"])
    # the Python host to step 2: the same boxes in State/Header (it holds nothing else that varies) and in every level's Cell_H
    nl, G = inputs.run(variant(plot_int=0), nsteps=2, report=None, outdir=str(py))
    try:
        assert G.istep == 2
    finally:
        G.close()
        gpu.initialize(params_for(WALLS), 0, 1, 0)
    assert open(str(a / "chk00002" / "State" / "Header")).read() == open(str(py / "chk00002" / "State" / "Header")).read()
    cf, cp = plotfile.read_checkfile(str(a / "chk00002")), plotfile.read_checkfile(str(py / "chk00002"))
    assert cf["dm"] == 2 and cf["boxes"] == cp["boxes"] and len(cf["boxes"]) == 2
    for sub in ("State", "Pressure"):
        for n in range(2):
            boxes = lambda root: open(os.path.join(root, "chk00002", sub, "Level_%02d" % n, "Cell_H")).read().split("FabOnDisk")[0]   # noqa: E731
            assert boxes(str(a)) == boxes(str(py)), (sub, n)
    # restarted from its own chk00002
    shutil.copytree(str(a / "chk00002"), str(b / "chk00002"))
    rows_b = _main("inputs", str(b))
    assert sorted(rows_b) == [3, 4]
    for s in (3, 4):
        (ta, da, ua), (tb, db, ub) = rows_a[s], rows_b[s]
        print("step %d: time %.17g vs %.17g, dt %.17g vs %.17g, |u|max %.17g vs %.17g" % (s, ta, tb, da, db, ua, ub))
        assert abs(ta - tb) <= 1e-12 * ta and abs(da - db) <= 1e-12 * da and abs(ua - ub) <= 1e-9 * ua
