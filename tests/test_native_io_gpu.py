"""Plot files and checkpoints written and read inside the library (varden_amd/csrc/fabio.hip: kk_fab_pack / kk_fab_unpack behind vdn_fabio_ml_multifab_write_d,
_read_d, vdn_checkpoint_write) against the Python writer of varden_amd/plotfile.py, which stays the definition of the format: every file byte for byte.
Small staging buffers (8 000 bytes) make the ranges of the pack / unpack launches end inside rows, components and fabs."""
import filecmp
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import WALLS, assert_bits, params_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# level 0: two boxes of different extents; level 1: two boxes whose three extents all differ, one 4 wide in x; no extent is a multiple of 8
L0 = [((0, 0, 0), (5, 6, 4)), ((6, 0, 0), (10, 6, 4))]
L1 = [((2, 2, 0), (5, 8, 4)), ((6, 2, 0), (15, 12, 8))]
PD = [((0, 0, 0), (10, 6, 4)), ((0, 0, 0), (21, 13, 9))]
L0_2D = [((0, 0, 0), (5, 6, 0)), ((6, 0, 0), (10, 6, 0))]
L1_2D = [((2, 2, 0), (5, 8, 0)), ((6, 2, 0), (15, 12, 0))]
PD_2D = [((0, 0, 0), (10, 6, 0)), ((0, 0, 0), (21, 13, 0))]
CASES = [(0, (0, 0, 0), 1), (3, (0, 0, 0), 5), (1, (1, 1, 1), 1)]
STAGING = [0, 8000]           # 0: the default (256 MB)
SENTINEL = -7.25e33


def same_tree(a, b, ignore=()):
    """every file of the two trees, byte for byte"""
    def files(root):
        return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs if f not in ignore)
    fa, fb = files(a), files(b)
    assert fa == fb and fa, (fa, fb)
    for f in fa:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), "%s differs between %s and %s" % (f, a, b)


class Tree:
    """a two-level hierarchy of seeded, non-zero, mixed-sign data on the device, ghost cells included"""

    def __init__(self, bl, dm, ng, nodal, nc, seed=3):
        self.bl, self.dm, self.ng, self.nc = bl, dm, ng, nc
        self.lists = [L0, L1] if dm == 3 else [L0_2D, L1_2D]
        self.pd = PD if dm == 3 else PD_2D
        self.nodal = tuple(nodal) if dm == 3 else tuple(nodal[:2]) + (0,)
        self.mla = bl.MLLayout(self.pd, self.lists, rr=[(2, 2, 2)])
        self.mfs = [bl.MultiFab(self.mla, n, nc, ng, self.nodal) for n in range(2)]
        rng = np.random.default_rng(seed)
        for mf in self.mfs:
            for i in range(mf.nfabs()):
                shp = mf.shape(i)
                mf.from_numpy(np.asfortranarray(rng.uniform(0.25, 3.0, size=shp) * rng.choice([-1.0, 1.0], size=shp)), i)

    def valid(self, a):
        g, gz = self.ng, self.ng if self.dm == 3 else 0
        return a[g:a.shape[0] - g, g:a.shape[1] - g, gz:a.shape[2] - gz]

    def levels(self, mfs=None):
        """what plotfile.write_ml_multifab takes: the valid slices of to_numpy"""
        return [dict(boxes=list(self.lists[n]), nodal=self.nodal, fabs=[self.valid(mf.to_numpy(i)).copy() for i in range(mf.nfabs())])
                for n, mf in enumerate(mfs or self.mfs)]

    def close(self):
        for m in self.mfs:
            m.destroy()
        self.mla.destroy()


def _byte_identity(bl, tmp_path, dm, ng, nodal, nc, staging):
    from varden_amd import advance as adv
    from varden_amd import plotfile
    T = Tree(bl, dm, ng, nodal, nc)
    try:
        lv = T.levels()
        assert all((a != 0).all() and (a < 0).any() and (a > 0).any() for L in lv for a in L["fabs"])
        # the defaults of both writers, then every optional argument given
        plotfile.write_ml_multifab(str(tmp_path / "py_a"), lv, [2], dm=dm)
        adv.fabio_ml_multifab_write_d(str(tmp_path / "lib_a"), T.mfs, [2], staging_bytes=staging)
        same_tree(str(tmp_path / "py_a"), str(tmp_path / "lib_a"))
        kw = dict(names=["q%d " % c for c in range(nc)], pd=T.pd[0], prob_lo=[-0.5, 0.25, 1.0][:dm], prob_hi=[1.7, 1.5, 3.0][:dm], time=0.1 + 0.2,
                  dx=[0.2, 0.125, 0.4][:dm])
        plotfile.write_ml_multifab(str(tmp_path / "py_b"), lv, [2], dm=dm, **kw)
        adv.fabio_ml_multifab_write_d(str(tmp_path / "lib_b"), T.mfs, [2], staging_bytes=staging, **kw)
        same_tree(str(tmp_path / "py_b"), str(tmp_path / "lib_b"))
        if staging:                                    # the small staging sizes cut the largest level into several ranges
            assert max(sum(a.size for a in L["fabs"]) for L in lv) * 8 > (8000 if dm == 3 else 800)
    finally:
        T.close()


@pytest.mark.parametrize("staging", STAGING)
@pytest.mark.parametrize("ng,nodal,nc", CASES)
def test_written_files_are_the_python_writers_3d(gpu, tmp_path, ng, nodal, nc, staging):
    gpu.initialize(params_for(WALLS), 0, 1, 0)
    _byte_identity(gpu, tmp_path, 3, ng, nodal, nc, staging)


@pytest.mark.parametrize("staging", STAGING + [800])          # (800 bytes: the 2-D levels are a few hundred points)
@pytest.mark.parametrize("ng,nodal,nc", CASES)
def test_written_files_are_the_python_writers_2d(gpu, tmp_path, ng, nodal, nc, staging):
    from tests.test_dim2_gpu import BC2, params2
    gpu.initialize(params2(BC2["walls"]), 0, 1, 0)
    try:
        _byte_identity(gpu, tmp_path, 2, ng, nodal, nc, staging)
    finally:
        gpu.initialize(params_for(WALLS), 0, 1, 0)                 # back to dm = 3 for the tests that follow


@pytest.mark.parametrize("staging", STAGING)
@pytest.mark.parametrize("ng,nodal,nc", CASES)
def test_read_fills_valid_points_and_leaves_ghost_cells(gpu, tmp_path, ng, nodal, nc, staging):
    from varden_amd import advance as adv
    gpu.initialize(params_for(WALLS), 0, 1, 0)
    T = Tree(gpu, 3, ng, nodal, nc)
    dst = [gpu.MultiFab(T.mla, n, nc + 1, ng, T.nodal) for n in range(2)]          # one component more than the file holds
    try:
        name = str(tmp_path / "tree")
        adv.fabio_ml_multifab_write_d(name, T.mfs, [2], staging_bytes=staging)
        for m in dst:
            m.setval(SENTINEL, all=True)
        adv.fabio_ml_multifab_read_d(name, dst, staging_bytes=staging)
        for n in range(2):
            for i in range(dst[n].nfabs()):
                got, want = dst[n].to_numpy(i), T.mfs[n].to_numpy(i)
                assert_bits(T.valid(got)[..., :nc], T.valid(want), "level %d box %d: valid points read back" % (n, i))
                untouched = np.ones(got.shape, dtype=bool)
                T.valid(untouched)[..., :nc] = False
                assert (got[untouched] == SENTINEL).all() and untouched.sum() == got.size - T.valid(want).size
    finally:
        for m in dst:
            m.destroy()
        T.close()


def test_read_refuses_other_boxes_and_short_files(gpu, tmp_path):
    from varden_amd import advance as adv
    from varden_amd.capi import VardenError
    gpu.initialize(params_for(WALLS), 0, 1, 0)
    T = Tree(gpu, 3, 1, (0, 0, 0), 2)
    other = [L0, [L1[0], ((6, 2, 0), (15, 12, 7))]]                               # box 1 of level 1 one plane shorter
    fewer = [L0, L1[:1]]                                                          # level 1 without its second box
    mla2, mla3 = gpu.MLLayout(PD, other, rr=[(2, 2, 2)]), gpu.MLLayout(PD, fewer, rr=[(2, 2, 2)])
    dst2 = [gpu.MultiFab(mla2, n, 2, 1) for n in range(2)] + [gpu.MultiFab(mla3, n, 2, 1) for n in range(2)]
    dst = [gpu.MultiFab(T.mla, n, 2, 1) for n in range(2)]
    dst2 += [gpu.MultiFab(T.mla, n, 2, 1, (1, 1, 1)) for n in range(2)] + [gpu.MultiFab(T.mla, n, 1, 1) for n in range(2)]
    name = str(tmp_path / "tree")
    try:
        adv.fabio_ml_multifab_write_d(name, T.mfs, [2])
        with pytest.raises(VardenError, match=r"level 1, box 1"):
            adv.fabio_ml_multifab_read_d(name, dst2[:2])
        with pytest.raises(VardenError, match=r"level 1: the file holds 2 boxes, the multifab 1"):
            adv.fabio_ml_multifab_read_d(name, dst2[2:4])
        with pytest.raises(VardenError, match=r"level 0.*nodal"):
            adv.fabio_ml_multifab_read_d(name, dst2[4:6])
        with pytest.raises(VardenError, match=r"level 0.*2 components.*1"):
            adv.fabio_ml_multifab_read_d(name, dst2[6:8])
        data = os.path.join(name, "Level_01", "Cell_D_00000")
        size = os.path.getsize(data)
        with open(data, "r+b") as f:
            f.truncate(size - 8)
        for staging in STAGING:
            with pytest.raises(VardenError, match=r"level 1, box 1.*Cell_D_00000.*cut short"):
                adv.fabio_ml_multifab_read_d(name, dst, staging_bytes=staging)
        # a FAB line that is not FAB_DESC
        raw = open(data, "rb").read()
        with open(data, "wb") as f:
            f.write(raw.replace(b"FAB ((8, (64 11 52", b"FAB ((4, (32  8 23", 1) + b"\0" * 8)
        with pytest.raises(VardenError, match=r"level 1, box 0.*Cell_D_00000.*FAB"):
            adv.fabio_ml_multifab_read_d(name, dst)
        gpu.MultiFab(T.mla, 0, 1, 0).destroy()                                    # the library still answers
    finally:
        for m in dst + dst2:
            m.destroy()
        mla2.destroy(); mla3.destroy()
        T.close()


def test_pieces_and_ranges_on_a_larger_box(gpu, tmp_path):
    """a (box, component) longer than the 4 096 values one workgroup moves, cut by 8 000-byte ranges: written like the Python writer writes it, read back whole"""
    from varden_amd import advance as adv
    from varden_amd import plotfile
    gpu.initialize(params_for(WALLS), 0, 1, 0)
    boxes = [((0, 0, 0), (20, 18, 16)), ((21, 0, 0), (27, 18, 16))]
    mla = gpu.MLLayout([((0, 0, 0), (27, 18, 16))], [boxes])
    src, dst = gpu.MultiFab(mla, 0, 2, 2), gpu.MultiFab(mla, 0, 2, 0)
    try:
        rng = np.random.default_rng(8)
        for i in range(2):
            src.from_numpy(np.asfortranarray(rng.standard_normal(src.shape(i)) + 0.01), i)
        fabs = [src.to_numpy(i)[2:-2, 2:-2, 2:-2].copy() for i in range(2)]
        assert fabs[0][..., 0].size > 4096
        plotfile.write_ml_multifab(str(tmp_path / "py"), [dict(boxes=boxes, fabs=fabs)], [], dm=3)
        adv.fabio_ml_multifab_write_d(str(tmp_path / "lib"), [src], [], staging_bytes=8000)
        same_tree(str(tmp_path / "py"), str(tmp_path / "lib"))
        adv.fabio_ml_multifab_read_d(str(tmp_path / "lib"), [dst], staging_bytes=8000)
        for i in range(2):
            assert_bits(dst.to_numpy(i), fabs[i], "box %d read back" % i)
    finally:
        src.destroy(); dst.destroy(); mla.destroy()


def test_several_ranks_are_refused(gpu, tmp_path):
    """one rank only: a process that initialised the library as one of two ranks gets the message, not a partial tree"""
    from varden_amd import advance as adv
    from varden_amd.capi import VardenError
    gpu.initialize(params_for(WALLS), 0, 2, 0)
    try:
        mla = gpu.MLLayout(PD[:1], [L0])
        mf = gpu.MultiFab(mla, 0, 1, 0)
        for call in (lambda: adv.fabio_ml_multifab_write_d(str(tmp_path / "t"), [mf], []), lambda: adv.fabio_ml_multifab_read_d(str(tmp_path / "t"), [mf]),
                     lambda: adv.checkpoint_write(str(tmp_path / "c"), [mf], [mf], [], 0.0, 0.0)):
            with pytest.raises(VardenError, match="several ranks: use the Python writer"):
                call()
        assert not os.path.exists(str(tmp_path / "t")) and not os.path.exists(str(tmp_path / "c"))
        mf.destroy(); mla.destroy()
    finally:
        gpu.initialize(params_for(WALLS), 0, 1, 0)


# ---- the drivers ------------------------------------------------------------------------------------------------------------------------------------
def _reference_plotfile(sim, name):
    """write_plotfile as the several-rank path still runs it: _gather + write_ml_multifab"""
    from varden_amd import advance as adv
    from varden_amd import boxlib as bl
    from varden_amd import plotfile as pf
    dm, ns = sim.dm, sim.nscal
    pd, nl = pf._domain(sim)
    ncomp = 2 * dm + ns + 2
    plot = [bl.MultiFab(sim.mla, n, ncomp, 0) for n in range(nl)]
    try:
        for n in range(nl):
            plot[n].copy_c(0, sim.uold[n], 0, dm)
            plot[n].copy_c(dm, sim.sold[n], 0, ns)
            adv.make_magvel(plot[n], dm + ns, sim.uold[n])
            adv.make_vorticity(plot[n], dm + ns + 1, sim.uold[n], sim.dx[n], sim.bct)
            plot[n].copy_c(dm + ns + 2, sim.gp[n], 0, dm)
        levels = pf._gather(sim, [plot])
    finally:
        for m in plot:
            m.destroy()
    dx0 = list(sim.dx[0][:dm])
    pf.write_ml_multifab(name, levels, [2] * (nl - 1), dm, pf.plot_names(dm, ns), pd, [0.0] * dm, [dx0[d] * (pd[1][d] + 1) for d in range(dm)], sim.time, dx0, nc=ncomp)


def _reference_checkfile(sim, name):
    from varden_amd import plotfile as pf
    pd, nl = pf._domain(sim)
    os.makedirs(name)
    pf.write_ml_multifab(os.path.join(name, "State"), pf._gather(sim, [sim.uold, sim.sold, sim.gp]), [2] * (nl - 1), sim.dm, pd=pd, nc=2 * sim.dm + sim.nscal)
    pf.write_ml_multifab(os.path.join(name, "Pressure"), pf._gather(sim, [sim.p], (1, 1, 1)), [2] * (nl - 1), sim.dm, pd=pd, nc=1)
    with open(os.path.join(name, "Header"), "w") as f:
        f.write("&CHKPOINT\n TIME=%s,\n DT=%s,\n NLEVS=%d,\n /\n" % (pf._es(sim.time).strip(), pf._es(sim.dt).strip(), nl))
        for _ in range(nl - 1):
            f.write("%12d\n" % 2)


@pytest.mark.parametrize("kind", ["one level", "two levels"])
def test_drivers_write_the_reference_paths_files_and_read_them_back(gpu, oracle, tmp_path, kind):
    from varden_amd import advance as adv
    from varden_amd import boxlib as bl
    from varden_amd import driver, plotfile
    if kind == "one level":
        G = driver.Varden(16, WALLS, params_for(WALLS, cflfac=0.9), init_shrink=0.1, init_iter=1)
    else:
        G = driver.VardenAMR(16, [((8, 8, 8), (23, 23, 23))], WALLS, params=params_for(WALLS, cflfac=0.9))
    try:
        G.step(); G.step()
        nl = plotfile._domain(G)[1]
        plt = plotfile.write_plotfile(G, base=str(tmp_path / "plt"))
        _reference_plotfile(G, str(tmp_path / "ref_plt"))
        same_tree(plt, str(tmp_path / "ref_plt"), ignore=("job_info",))
        assert os.path.exists(os.path.join(plt, "job_info"))
        chk = plotfile.write_checkfile(G, base=str(tmp_path / "chk"))
        _reference_checkfile(G, str(tmp_path / "ref_chk"))
        same_tree(chk, str(tmp_path / "ref_chk"))
        # vdn_checkpoint_info + _info / _boxes + _read_d against read_checkfile
        c = plotfile.read_checkfile(chk)
        assert adv.checkpoint_info(chk) == dict(nlevs=c["nlevs"], time=c["time"], dt=c["dt"], rr=c["rr"]) and c["nlevs"] == nl
        for sub, key, nodal in (("State", "state", (0, 0, 0)), ("Pressure", "pressure", (1, 1, 1))):
            d = os.path.join(chk, sub)
            info = adv.fabio_ml_multifab_info(d)
            assert info["nlevs"] == nl and info["nodal"] == nodal and info["dm"] == 3 and info["ncomp"] == c[key][0][0].shape[3]
            boxes = [adv.fabio_ml_multifab_boxes(d, n, info["nboxes"][n]) for n in range(nl)]
            assert boxes == c["boxes"]
            mla = bl.MLLayout([((0, 0, 0), (16 * 2 ** n - 1,) * 3) for n in range(nl)], boxes, rr=[(2, 2, 2)] * (nl - 1))
            mfs = [bl.MultiFab(mla, n, info["ncomp"], 2, nodal) for n in range(nl)]
            try:
                adv.fabio_ml_multifab_read_d(d, mfs)
                for n in range(nl):
                    for i in range(mfs[n].nfabs()):
                        assert_bits(mfs[n].to_numpy(i)[2:-2, 2:-2, 2:-2], c[key][n][i], "%s level %d box %d" % (sub, n, i))
            finally:
                for m in mfs:
                    m.destroy()
                mla.destroy()
    finally:
        G.close()


# ---- the Fortran host -------------------------------------------------------------------------------------------------------------------------------
MAIN = os.path.join(ROOT, "varden_amd", "fortran", "varden_main")
STEP = re.compile(r"\s*step\s+(\d+)\s+time\s+(\S+)\s+dt\s+(\S+)")


def _main(inputs_path, cwd):
    out = subprocess.run([MAIN, inputs_path], cwd=cwd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return {int(STEP.match(ln).group(1)): ln for ln in out.stdout.splitlines() if STEP.match(ln)}


def test_fortran_main_writes_plot_files_and_restarts_from_its_checkpoint(gpu, tmp_path):
    from varden_amd import inputs, plotfile
    if not os.path.exists(MAIN):
        if shutil.which("amdflang") is None and not os.path.exists("/opt/rocm/lib/llvm/bin/flang"):
            pytest.skip("no flang on this box and no prebuilt varden_main")
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(MAIN)])
    text = open(os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d")).read()

    def variant(**kw):
        t = text
        for k, v in kw.items():
            t, n = re.subn(r"(?mi)^(\s*%s\s*=\s*)[^!\n]*" % k, lambda m: m.group(1) + str(v) + " ", t)
            if n == 0:
                t = re.sub(r"(?m)^\s*/\s*$", " %s = %s\n/" % (k, v), t, count=1)
        return t
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(); b.mkdir()
    (a / "inputs").write_text(variant(max_step=4, chk_int=2, plot_int=2))
    (b / "inputs").write_text(variant(max_step=4, chk_int=2, plot_int=2, restart=2))
    rows_a = _main("inputs", str(a))
    shutil.copytree(str(a / "chk00002"), str(b / "chk00002"))
    rows_b = _main("inputs", str(b))
    assert sorted(rows_a) == [1, 2, 3, 4] and sorted(rows_b) == [3, 4]
    assert rows_b[3] == rows_a[3] and rows_b[4] == rows_a[4]
    same_tree(str(a / "chk00004"), str(b / "chk00004"))
    assert sorted(p for p in os.listdir(str(a)) if p[:3] in ("plt", "chk")) == ["chk00000", "chk00002", "chk00004", "plt00000", "plt00002", "plt00004"]
    r = plotfile.read_ml_multifab(str(a / "plt00002"))
    assert r["names"] == plotfile.plot_names(3, 2) and all(f.shape[3] == 10 for L in r["levels"] for f in L["fabs"])
    # the Python host restarted from the Fortran host's checkpoint reaches its step 4
    m = STEP.match(rows_a[4])
    nl, G = inputs.run(variant(max_step=4, chk_int=0, plot_int=0, restart=2), nsteps=4, outdir=str(a))
    try:
        assert G.istep == 4
        assert abs(G.time - float(m.group(2))) <= 1e-12 * G.time and abs(G.dt - float(m.group(3))) <= 1e-12 * G.dt, (G.time, G.dt, rows_a[4])
    finally:
        G.close()
