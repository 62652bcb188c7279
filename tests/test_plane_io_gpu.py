"""The files of a 2-D hierarchy that runs as its z-uniform 3-D copy: plane k = 0 written as a dm = 2 hierarchy inside the library
(vdn_fabio_ml_multifab_write_plane_d, vdn_checkpoint_write_plane: kk_fab_pack on plane segments, kk_plane_defect), read back into every plane of a copy
(vdn_fabio_ml_multifab_read_plane_d: kk_fab_unpack_extrude), the vorticity by makevort_2d's rule on every plane (vdn_make_vorticity_plane) -- against the Python
writer of varden_amd/plotfile.py and the 2-D oracle, bit for bit; then the drivers: run, write, restart, fixed_grids."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

from tests.test_native_io_gpu import same_tree
from tests.util import WALLS, assert_bits, params_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# level 0: two footprints of different extents, z = 0..7 cut into 0..3 and 4..7; level 1: two footprints whose extents all differ, one 4 wide in x, z = 0..15 cut into the
# uneven 0..8 and 9..15; no extent is a multiple of 8
FP = [[((0, 0), (5, 6)), ((6, 0), (10, 6))], [((2, 2), (5, 8)), ((6, 2), (15, 12))]]
ZCUT = [[(0, 3), (4, 7)], [(0, 8), (9, 15)]]
ZCUT_OTHER = [[(0, 7)], [(0, 4), (5, 9), (10, 15)]]          # what the reader's multifabs are cut into (a layout takes no box narrower than 4 cells)
PD = [((0, 0, 0), (10, 6, 7)), ((0, 0, 0), (21, 13, 15))]
CASES = [(0, (0, 0, 0), 1), (3, (0, 0, 0), 5), (1, (1, 1, 1), 5), (1, (1, 1, 1), 1)]
STAGING = [0, 8000, 800]          # 0: the default; the others end the ranges inside rows, components and fabs
SENTINEL = -7.25e33
COMPS5 = [0, 1, 3, 4]             # of five components; component 2 is the one that must vanish


def boxes3d(fps, zcut):
    return [((lo[0], lo[1], z0), (hi[0], hi[1], z1)) for z0, z1 in zcut for lo, hi in fps]


def boxes2d(fps):
    return [((lo[0], lo[1], 0), (hi[0], hi[1], 0)) for lo, hi in fps]


class Copy:
    """a two-level z-uniform copy on the device: seeded, non-zero, mixed-sign planes, the same on every valid plane of every box of a footprint; ghost cells hold other values;
    with five components, component 2 is zero on the valid points"""

    def __init__(self, bl, ng, nodal, nc, zcut=ZCUT, seed=3, fill=True):
        self.bl, self.ng, self.nc, self.nodal = bl, ng, nc, tuple(nodal)
        self.lists = [boxes3d(FP[n], zcut[n]) for n in range(2)]
        self.mla = bl.MLLayout(PD, self.lists, rr=[(2, 2, 2)])
        self.mfs = [bl.MultiFab(self.mla, n, nc, ng, self.nodal) for n in range(2)]
        rng = np.random.default_rng(seed)
        nd = self.nodal
        self.planes = [[rng.uniform(0.25, 3.0, size=(hi[0] - lo[0] + 1 + nd[0], hi[1] - lo[1] + 1 + nd[1], 1, nc)) *
                        rng.choice([-1.0, 1.0], size=(hi[0] - lo[0] + 1 + nd[0], hi[1] - lo[1] + 1 + nd[1], 1, nc)) for lo, hi in FP[n]] for n in range(2)]
        if nc == 5:
            for pl in self.planes:
                for p in pl:
                    p[..., 2] = 0.0
        if fill:
            for n, mf in enumerate(self.mfs):
                for i in range(mf.nfabs()):
                    a = np.asfortranarray(rng.uniform(4.0, 5.0, size=mf.shape(i)))
                    self.valid(a)[...] = self.planes[n][i % len(FP[n])]
                    mf.from_numpy(a, i)

    def valid(self, a):
        g = self.ng
        return a[g:a.shape[0] - g, g:a.shape[1] - g, g:a.shape[2] - g]

    def levels(self, comps):
        """what plotfile.write_ml_multifab(dm=2) takes: the planes"""
        return [dict(boxes=boxes2d(FP[n]), nodal=self.nodal[:2] + (0,), fabs=[np.ascontiguousarray(p[..., comps]) for p in self.planes[n]]) for n in range(2)]

    def close(self):
        for m in self.mfs:
            m.destroy()
        self.mla.destroy()


def _comps(nc):
    return (COMPS5, [2]) if nc == 5 else ([0], [])


@pytest.mark.parametrize("staging", STAGING)
@pytest.mark.parametrize("ng,nodal,nc", CASES)
def test_plane_files_are_the_python_writers(gpu, tmp_path, ng, nodal, nc, staging):
    from varden_amd import advance as adv
    from varden_amd import plotfile
    gpu.initialize(params_for(WALLS), 0, 1, 0)
    T = Copy(gpu, ng, nodal, nc)
    try:
        comps, vanish = _comps(nc)
        lv = T.levels(comps)
        assert all((a != 0).all() and (a < 0).any() and (a > 0).any() for L in lv for a in L["fabs"])
        # the defaults of both writers, then every optional argument given
        plotfile.write_ml_multifab(str(tmp_path / "py_a"), lv, [2], dm=2)
        d = adv.fabio_ml_multifab_write_plane_d(str(tmp_path / "lib_a"), T.mfs, [2], comps, staging_bytes=staging, vanish=vanish)
        same_tree(str(tmp_path / "py_a"), str(tmp_path / "lib_a"))
        assert d == (0.0, 0.0), d
        kw = dict(names=["q%d " % c for c in comps], pd=((0, 0, 0), (10, 6, 0)), prob_lo=[-0.5, 0.25], prob_hi=[1.7, 1.5], time=0.1 + 0.2, dx=[0.2, 0.125])
        plotfile.write_ml_multifab(str(tmp_path / "py_b"), lv, [2], dm=2, **kw)
        assert adv.fabio_ml_multifab_write_plane_d(str(tmp_path / "lib_b"), T.mfs, [2], comps, staging_bytes=staging, defect=False, **kw) is None
        same_tree(str(tmp_path / "py_b"), str(tmp_path / "lib_b"))
        if staging == 800:                                                             # cuts every level into several ranges (8 000 bytes hold a whole level of these planes)
            assert max(sum(a.size for a in L["fabs"]) for L in lv) * 8 > staging
        r = plotfile.read_ml_multifab(str(tmp_path / "lib_b"))
        assert r["dm"] == 2 and [L["boxes"] for L in r["levels"]] == [boxes2d(f) for f in FP] and r["levels"][0]["nodal"] == T.nodal[:2] + (0,)
    finally:
        T.close()


@pytest.mark.parametrize("staging", STAGING)
@pytest.mark.parametrize("ng,nodal,nc", CASES)
def test_read_spreads_the_plane_over_every_valid_plane(gpu, tmp_path, ng, nodal, nc, staging):
    from varden_amd import advance as adv
    gpu.initialize(params_for(WALLS), 0, 1, 0)
    T = Copy(gpu, ng, nodal, nc)
    D = Copy(gpu, ng, nodal, nc, zcut=ZCUT_OTHER, fill=False)                          # cut along z differently from the writer
    try:
        comps, _ = _comps(nc)
        name = str(tmp_path / "planes")
        adv.fabio_ml_multifab_write_plane_d(name, T.mfs, [2], comps, staging_bytes=staging, defect=False)
        for m in D.mfs:
            m.setval(SENTINEL, all=True)
        adv.fabio_ml_multifab_read_plane_d(name, D.mfs, comps, staging_bytes=staging)
        for n in range(2):
            for i in range(D.mfs[n].nfabs()):
                got = D.mfs[n].to_numpy(i)
                lo, hi = D.lists[n][i]
                v = D.valid(got)
                assert v.shape[2] == hi[2] - lo[2] + 1 + nodal[2]
                plane = T.planes[n][i % 2][..., comps]
                for k in range(v.shape[2]):                                             # (the top node plane included)
                    assert_bits(v[:, :, k:k + 1, :][..., comps], plane, "level %d box %d plane %d" % (n, i, k))
                untouched = np.ones(got.shape, dtype=bool)
                D.valid(untouched)[..., comps] = False
                assert (got[untouched] == SENTINEL).all() and untouched.sum() == got.size - v[..., comps].size
    finally:
        D.close(); T.close()


def test_defect_report_sees_a_plane_that_differs_and_a_component_that_does_not_vanish(gpu, tmp_path):
    from varden_amd import advance as adv
    gpu.initialize(params_for(WALLS), 0, 1, 0)
    T = Copy(gpu, 1, (0, 0, 0), 5)
    try:
        # level 1, box 3 = footprint 1 in the chunk z = 9..15, which does not hold k = 0: one value of component 3 moves by 2^-20
        a = T.mfs[1].to_numpy(3)
        old = a[1 + 4, 1 + 7, 1 + 2, 3]
        a[1 + 4, 1 + 7, 1 + 2, 3] = old + 2.0 ** -20
        want = abs(a[1 + 4, 1 + 7, 1 + 2, 3] - old)
        assert want > 0 and old == T.planes[1][1][4, 7, 0, 3]
        T.mfs[1].from_numpy(a, 3)
        d = adv.fabio_ml_multifab_write_plane_d(str(tmp_path / "a"), T.mfs, [2], COMPS5, vanish=[2])
        assert d == (want, 0.0), (d, want)
        # the files are still those of plane k = 0, which was not touched
        T2 = Copy(gpu, 1, (0, 0, 0), 5)
        try:
            adv.fabio_ml_multifab_write_plane_d(str(tmp_path / "b"), T2.mfs, [2], COMPS5, defect=False)
        finally:
            T2.close()
        same_tree(str(tmp_path / "a"), str(tmp_path / "b"))
        # level 0, box 2 (z = 4..7): one value of the component that must vanish
        b = T.mfs[0].to_numpy(2)
        b[1 + 3, 1 + 5, 1 + 1, 2] = -0.375
        T.mfs[0].from_numpy(b, 2)
        d = adv.fabio_ml_multifab_write_plane_d(str(tmp_path / "c"), T.mfs, [2], COMPS5, vanish=[2], staging_bytes=800)
        assert d == (want, 0.375), (d, want)
        # the same figures from the checkpoint writer (State = the listed components, Pressure = component 0 of a second hierarchy)
        d = adv.checkpoint_write_plane(str(tmp_path / "chk"), T.mfs, T.mfs, [2], 0.5, 0.25, COMPS5, vanish=[2])
        assert d == (want, 0.375), (d, want)
        assert adv.checkpoint_info(str(tmp_path / "chk")) == dict(nlevs=2, time=0.5, dt=0.25, rr=[2])
        same_tree(str(tmp_path / "chk" / "State"), str(tmp_path / "b"), ignore=("Header",))          # (the Header of a checkpoint's State has its own defaults)
        info = adv.fabio_ml_multifab_info(str(tmp_path / "chk" / "Pressure"))
        assert info["dm"] == 2 and info["ncomp"] == 1 and info["nboxes"] == [2, 2]
    finally:
        T.close()


def test_footprints_that_do_not_match_are_refused(gpu, tmp_path):
    from varden_amd import advance as adv
    from varden_amd.capi import VardenError
    gpu.initialize(params_for(WALLS), 0, 1, 0)
    T = Copy(gpu, 1, (0, 0, 0), 5)
    l1 = list(T.lists[1])
    l1[3] = ((6, 2, 9), (14, 12, 15))                                                # box 3 of level 1 one cell narrower than the box below it
    mla2 = gpu.MLLayout(PD, [T.lists[0], l1], rr=[(2, 2, 2)])
    bad = [gpu.MultiFab(mla2, n, 5, 1) for n in range(2)]
    l1o = [((6, 2, 0), (15, 12, 15)), ((2, 2, 0), (5, 8, 15)), ((2, 2, 0), (5, 9, 15))]     # overlapping footprints, both at k = 0
    mla3 = gpu.MLLayout(PD, [T.lists[0], l1o], rr=[(2, 2, 2)])
    bad3 = [gpu.MultiFab(mla3, n, 5, 1) for n in range(2)]
    try:
        with pytest.raises(VardenError, match=r"level 1, box 3.*footprint \(6,2\)-\(14,12\)"):
            adv.fabio_ml_multifab_write_plane_d(str(tmp_path / "w"), bad, [2], COMPS5)
        with pytest.raises(VardenError, match=r"level 1, box 2.*overlaps.*box 1"):
            adv.fabio_ml_multifab_write_plane_d(str(tmp_path / "w"), bad3, [2], COMPS5)
        with pytest.raises(VardenError, match=r"level 1, box 3"):
            adv.checkpoint_write_plane(str(tmp_path / "w"), bad, bad, [2], 0.0, 0.0, COMPS5)
        assert not os.path.exists(str(tmp_path / "w"))                                # refused before anything was written
        name = str(tmp_path / "planes")
        adv.fabio_ml_multifab_write_plane_d(name, T.mfs, [2], COMPS5, defect=False)
        with pytest.raises(VardenError, match=r"level 1, box 3.*footprint \(6,2\)-\(14,12\)"):
            adv.fabio_ml_multifab_read_plane_d(name, bad, COMPS5)
        with pytest.raises(VardenError, match=r"4 components, 3 were named"):
            adv.fabio_ml_multifab_read_plane_d(name, T.mfs, COMPS5[:3])
        # a plane file is not a file of a dm = 3 run: fabio_ml_multifab_read_d fails as it always has
        with pytest.raises(VardenError, match=r"is 2-dimensional, the run 3-dimensional"):
            adv.fabio_ml_multifab_read_d(name, T.mfs)
        # ... and a 3-D file is not a plane file
        adv.fabio_ml_multifab_write_d(str(tmp_path / "full"), T.mfs, [2])
        with pytest.raises(VardenError, match=r"is 3-dimensional, not a plane file"):
            adv.fabio_ml_multifab_read_plane_d(str(tmp_path / "full"), T.mfs, list(range(5)))
        gpu.MultiFab(T.mla, 0, 1, 0).destroy()                                        # the library still answers
    finally:
        for m in bad + bad3:
            m.destroy()
        mla2.destroy(); mla3.destroy()
        T.close()


@pytest.mark.parametrize("bcname", ["walls", "slip", "periodic", "inout", "outin-y"])
def test_vorticity_plane_is_makevort_2d_on_every_plane(gpu, oracle, bcname):
    from tests.test_dim2_gpu import BC2, Case2, _prm_pair
    from varden_amd import advance as adv
    bc = BC2[bcname]
    nx, ny, nz = 24, 20, 4
    try:
        K = Case2((nx, ny), bc, seed=12)
        u, _ = K.random_state()
        ov = K.ofab(0, 2)
        oracle.lib().vo_makevort(ov.ref, 1, u.ref, K.odx, C.byref(K.obc))
        dx = list(K.dx)
        K.close()
        want = ov.a[:, :, 0, 1]
        assert (want < 0).any() and (want > 0).any()
        gpu.initialize(_prm_pair(bc)[1], 0, 1, 0)
        phys3 = [list(bc[0]), list(bc[1]), [-1, -1]]
        box = ((0, 0, 0), (nx - 1, ny - 1, nz - 1))
        mla = gpu.MLLayout([box], [[box]], pmask=[1 if p[0] == -1 else 0 for p in phys3])
        bct = gpu.BCTower(mla, phys3)
        gu, gv = gpu.MultiFab(mla, 0, 3, 3), gpu.MultiFab(mla, 0, 2, 0)
        try:
            a = np.zeros(gu.shape(0), order="F")
            a[..., :2] = np.where(np.isfinite(u.a), u.a, 0.0)[:, :, 0, None, :]          # the same (u, v) on every plane, ghost planes included; w = 0
            gu.from_numpy(a)
            gv.setval(SENTINEL, all=True)
            adv.make_vorticity_plane(gv, 1, gu, dx, bct)
            got = gv.to_numpy()
            for k in range(nz):
                assert_bits(got[:, :, k, 1], want, "%s: plane %d" % (bcname, k))
            assert (got[..., 0] == SENTINEL).all()
        finally:
            gu.destroy(); gv.destroy(); bct.destroy(); mla.destroy()
    finally:
        gpu.initialize(params_for(WALLS), 0, 1, 0)                                    # back to the defaults for the tests that follow


# ---- the drivers: run, write, restart ------------------------------------------------------------------------------------------------------------------
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_2d_n32_chk")
NZ = 16


def variant(**kw):
    t = open(INPUTS).read()
    for k, v in kw.items():
        t, n = re.subn(r"(?mi)^(\s*%s\s*=\s*)[^!\n]*" % k, lambda m: m.group(1) + str(v) + " ", t)
        if n == 0:
            t = re.sub(r"(?m)^\s*/\s*$", " %s = %s\n/" % (k, v), t, count=1)
    return t


def planes_of(G):
    """plane k = 0 of the carried state as level-domain arrays (NaN outside the level's boxes): u, v | rho, tracer | gpx, gpy | the nodal p"""
    u, s, gp = G.slice2d(G.uold), G.slice2d(G.sold), G.slice2d(G.gp)
    p = []
    for n, mf in enumerate(G.p):
        a = np.full(((G.ncs[0] << n) + 1, (G.ncs[1] << n) + 1, 1), np.nan)
        for li, gi in enumerate(G.local[n]):
            lo, hi = G.boxes[n][gi]
            if lo[2] == 0:
                f = mf.to_numpy(li)
                a[lo[0]:hi[0] + 2, lo[1]:hi[1] + 2, :] = f[1:-1, 1:-1, 1, :]
        p.append(a)
    return dict(u=[x[..., :2] for x in u], s=s, gp=[x[..., :2] for x in gp], p=p, w=[x[..., 2:] for x in u], gpz=[x[..., 2:] for x in gp])


@pytest.fixture(scope="module")
def run_a(gpu, tmp_path_factory):
    """run A: four steps of the 2-D bubble as a 32 x 32 x 16 copy with one refined level (cut in two along z), plot files every second step, a checkpoint every step"""
    from varden_amd import inputs
    out = tmp_path_factory.mktemp("run_a")
    seen = {}

    def rep(G):
        seen[G.istep] = dict(planes=planes_of(G), boxes=[list(b) for b in G.boxes], time=G.time, dt=G.dt)
    nl, G = inputs.run(variant(grids_file_name="'grids'"), report=rep, outdir=str(out), extrude_nz=NZ)
    try:
        assert G.extrude2d == NZ and G.istep == 4 and G.nlev == 2
        defect = G.last_copy_defect
    finally:
        G.close()
        gpu.initialize(params_for(WALLS), 0, 1, 0)
    return dict(out=str(out), seen=seen, defect=defect)


def test_a_2d_hierarchy_writes_the_2d_runs_files(gpu, run_a):
    from varden_amd import plotfile
    out, at2 = run_a["out"], run_a["seen"][2]
    assert sorted(p for p in os.listdir(out) if p[:3] in ("plt", "chk")) == ["chk0000%d" % i for i in range(5)] + ["plt00000", "plt00002", "plt00004"]
    assert any(lo[2] > 0 for lo, _ in at2["boxes"][1]), "level 1 is not cut along z"
    r = plotfile.read_ml_multifab(os.path.join(out, "plt00002"))
    assert r["dm"] == 2 and r["names"] == plotfile.plot_names(2, 2) and r["nlevs"] == 2 and r["time"] == at2["time"]
    assert r["pd"] == ((0, 0, 0), (31, 31, 0)) and r["prob_hi"] == [1.0, 1.0] and r["dx"] == [1.0 / 32] * 2
    pl = at2["planes"]
    vort = []
    for n in range(2):
        assert r["levels"][n]["boxes"] == plotfile.footprints(at2["boxes"][n])[0]
        for (lo, hi), f in zip(r["levels"][n]["boxes"], r["levels"][n]["fabs"]):
            sl = (slice(lo[0], hi[0] + 1), slice(lo[1], hi[1] + 1))
            assert f.shape == (hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, 1, 8)
            assert_bits(f[:, :, 0, 0:2], pl["u"][n][sl], "plt00002 level %d: velocity" % n)
            assert_bits(f[:, :, 0, 2:4], pl["s"][n][sl], "plt00002 level %d: scalars" % n)
            assert_bits(f[:, :, 0, 6:8], pl["gp"][n][sl], "plt00002 level %d: grad p" % n)
            mag = np.sqrt(pl["u"][n][sl][..., 0] ** 2 + pl["u"][n][sl][..., 1] ** 2)
            assert np.abs(f[:, :, 0, 4] - mag).max() <= 1e-14 * max(mag.max(), 1e-3)
            vort.append(f[:, :, 0, 5])
    assert min(v.min() for v in vort) < 0 < max(v.max() for v in vort)
    assert len(re.findall(r"(?m)^   -[xyz]:", open(os.path.join(out, "plt00002", "job_info")).read())) == 2          # two directions
    c = plotfile.read_checkfile(os.path.join(out, "chk00002"))
    assert c["dm"] == 2 and c["boxes"] == [L["boxes"] for L in r["levels"]] and c["time"] == at2["time"] and c["dt"] == at2["dt"]
    for n in range(2):
        for (lo, hi), st, pr in zip(c["boxes"][n], c["state"][n], c["pressure"][n]):
            sl = (slice(lo[0], hi[0] + 1), slice(lo[1], hi[1] + 1))
            assert_bits(st[:, :, 0, :], np.concatenate([pl["u"][n][sl], pl["s"][n][sl], pl["gp"][n][sl]], axis=2), "chk00002 level %d: State" % n)
            assert_bits(pr[:, :, 0, :], pl["p"][n][lo[0]:hi[0] + 2, lo[1]:hi[1] + 2], "chk00002 level %d: Pressure" % n)
    # the writer said how far the copy is from z-uniform (reported, not judged: the restart test prints the figures)
    assert all(np.isfinite(d) and d >= 0.0 for d in run_a["defect"]), run_a["defect"]


@pytest.mark.parametrize("restart", [2, 3])          # 2: the next step regrids; 3: the next step runs on the boxes rebuilt from the file
def test_a_2d_hierarchy_restarts_from_its_plane_checkpoint(gpu, run_a, tmp_path, restart):
    """Run A against a run restarted from A's chk<restart> and taken to step 4: time and dt to 1e-12 relative, plane k = 0 of u, v, rho, tracer, grad p and p to 1e-9 of each
    field's scale.  A restart replaces every plane by plane 0, a perturbation of the size the copy's planes differ by (1e-10 of scale: tests/test_dim2_gpu.py), hence the project's
    end-to-end bound and not bits.  The measured differences are printed (profiles/plane_io_restart.txt keeps a copy)."""
    from varden_amd import inputs
    shutil.copytree(os.path.join(run_a["out"], "chk%05d" % restart), str(tmp_path / ("chk%05d" % restart)))
    nl, G = inputs.run(variant(restart=restart, plot_int=0, chk_int=0), report=None, outdir=str(tmp_path), extrude_nz=NZ)
    try:
        assert G.istep == 4 and G.extrude2d == NZ
        A = run_a["seen"][4]
        print("restart = %d: last_copy_defect of run A = (%.3e, %.3e)" % ((restart,) + tuple(run_a["defect"])))
        print("restart = %d: time %.17g vs %.17g, dt %.17g vs %.17g" % (restart, G.time, A["time"], G.dt, A["dt"]))
        got = planes_of(G)
        worst = {}
        for key in ("u", "s", "gp", "p"):
            for n in range(2):
                a, b = A["planes"][key][n], got[key][n]
                assert (np.isfinite(a) == np.isfinite(b)).all(), "restart = %d: level %d covers other cells" % (restart, n)
                m = np.isfinite(a)
                scale = max(max(np.nanmax(np.abs(x)) for x in A["planes"][key]), 1e-3)
                worst[key] = max(worst.get(key, 0.0), np.abs(a[m] - b[m]).max() / scale)
            print("restart = %d: max |%s - %s of run A| / scale = %.3e" % (restart, key, key, worst[key]))
        zero = max(np.nanmax(np.abs(x)) for k in ("w", "gpz") for x in got[k])
        print("restart = %d: max |w|, |gpz| on plane 0 at step 4 = %.3e" % (restart, zero))
        assert abs(G.time - A["time"]) <= 1e-12 * A["time"] and abs(G.dt - A["dt"]) <= 1e-12 * A["dt"]
        for key, v in worst.items():
            assert v <= 1e-9, (restart, key, v)
    finally:
        G.close()
        gpu.initialize(params_for(WALLS), 0, 1, 0)


def test_fixed_grids_of_a_2d_hierarchy(gpu, run_a, tmp_path):
    from varden_amd import advance as adv, inputs, plotfile
    shutil.copy(os.path.join(run_a["out"], "grids"), str(tmp_path / "grids"))
    step0 = [L["boxes"] for L in plotfile.read_ml_multifab(os.path.join(run_a["out"], "plt00000"))["levels"]]
    assert plotfile.read_grids(str(tmp_path / "grids"))[1] == step0

    def rep(G):
        assert adv.last_solver_stats("mac")[2] <= 1e-10 * adv.last_solver_stats("mac")[1] and adv.last_solver_stats("hg")[0] < 60
        assert [plotfile.footprints(b)[0] for b in G.boxes] == step0
    nl, G = inputs.run(variant(fixed_grids="'grids'", regrid_int=-1, plot_int=0, chk_int=0, max_step=2), report=rep, outdir=str(tmp_path), extrude_nz=NZ)
    try:
        assert G.istep == 2 and G.extrude2d == NZ and G.nlev == 2 and G.nregrids == 0
        assert G.boxes[1] == plotfile.extrude_boxes(step0[1], 2 * NZ, 16) and len(G.boxes[1]) == 2 * len(step0[1])
        u = G.slice2d(G.uold)
        assert all(np.isfinite(x[np.isfinite(x)]).all() for x in u) and max(np.nanmax(np.abs(x)) for x in u) > 0
    finally:
        G.close()
        gpu.initialize(params_for(WALLS), 0, 1, 0)
