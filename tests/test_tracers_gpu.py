"""Extra tracers: nscal up to 11 through advance_timestep (src/_parameters: nscal; every stage of the reference loops over components 2 .. nscal).
The scalar Godunov kernels take at most three components per launch, so the scalars run in windows of three (godunov.hip: k_mkflux, comp_window).
Held against the oracle on one level and on box-list hierarchies, against the library itself bit for bit (a tracer does not feel the others:
passivity pins the windows), over several ranks, through restart, plot files, the inputs driver and the Fortran host."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.children import launch_ranks
from tests._tracers_worker import FIVE, init_with_tracers, set_tracers
from tests.util import INOUT, PER, WALLS, assert_bits, params_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. one level against the oracle ---------------------------------------------------------------------------------------------------------------
def _one_level_pair(n, phys, prob, nscal, nsteps, **kw):
    """the same start-up sequence on both sides (initial projection, first dt, one pressure iteration) from initdata with the tracers 2 .. nscal - 1
    set to tracer_value; returns (oracle, library) after nsteps steps, dt / V-cycle counts checked in every step"""
    from oracle import voracle as vo
    from varden_amd import advance as adv
    from varden_amd import driver
    fields = FIVE[:nscal - 1]
    O = vo.Sim(n, phys, params_for(phys, cflfac=0.9, nscal=nscal, **kw), prob_type=prob, init_shrink=0.1, init_iter=0)
    ou, os_ = vo.Fab((0, 0, 0), (n - 1,) * 3, 3, 3), vo.Fab((0, 0, 0), (n - 1,) * 3, 3, nscal)
    vo.lib().vo_initdata(ou.ref, os_.ref, O.dx, prob)
    s0 = os_.a.copy(order="F")
    t1 = s0[..., 1].copy()
    set_tracers(s0, (0, 0, 0), [1.0 / n] * 3, fields)
    s0[..., 1] = t1                                          # tracer 1 keeps initdata's field, 2 .. get theirs
    g = 3
    assert np.array_equal(O.sold.valid()[..., :2], s0[g:-g, g:-g, g:-g, :2])
    O.sold.a[...] = s0                                       # the oracle's start-up with init_iter = 1, the tracers put in before the pressure iteration
    O.fill_state_ghosts()
    O.snew.a[...] = O.sold.a
    O.advance(vo.PRESSURE_ITERS)
    G = driver.Varden(n, phys, params_for(phys, cflfac=0.9, nscal=nscal, **kw), prob_type=prob, init_shrink=0.1, init_iter=1, u0=ou.a, s0=s0)
    assert G.dt == O.dt
    for step in range(nsteps):
        O.step(); G.step()
        assert G.dt == O.dt, "dt diverged at step %d: %r vs %r" % (step, G.dt, O.dt)
        cg = (adv.last_solver_stats("mac")[0], adv.last_solver_stats("hg")[0])
        assert cg == (O.mgstat[0].cycles, O.mgstat[1].cycles), "step %d: V-cycle counts %r vs %r" % (step, cg, (O.mgstat[0].cycles, O.mgstat[1].cycles))
    return O, G


def _check_fields(O, G, what):
    g = 3
    a, b = G.unew[0].to_numpy()[g:-g, g:-g, g:-g], O.unew.valid()
    scale = max(float(np.abs(b).max()), 1e-300)
    assert np.abs(a - b).max() <= 1e-9 * scale, "%s: u differs by %.3e (scale %.3e)" % (what, np.abs(a - b).max(), scale)
    a, b = G.snew[0].to_numpy()[g:-g, g:-g, g:-g], O.snew.valid()
    for c in range(b.shape[3]):
        scale = float(np.abs(b[..., c]).max())
        err = float(np.abs(a[..., c] - b[..., c]).max())
        assert scale > 0.05 and err <= 1e-9 * scale, "%s: scalar %d differs by %.3e (scale %.3e)" % (what, c, err, scale)


@pytest.mark.parametrize("n,name,phys,prob", [(16, "walls", WALLS, 1), (16, "periodic", PER, 1), (16, "inout", INOUT, 2),
                                              (32, "walls", WALLS, 1), (32, "inout", INOUT, 2)])
def test_five_scalars_against_the_oracle(gpu, oracle, n, name, phys, prob):
    """nscal = 5: the density and four tracers, three of them with fields of their own.  At the inflow face (inout) the reference sets rho_bc and trac_bc
    only (multifab_physbc.f90:98-99): the tracers 2 .. keep their extrapolated ghost values on both sides."""
    O, G = _one_level_pair(n, phys, prob, 5, 3)
    _check_fields(O, G, "%d^3 %s" % (n, name))
    G.close()


@pytest.mark.parametrize("name,phys,prob,dtype", [("walls-CN", WALLS, 1, 1), ("inout-BE", INOUT, 2, 2)])
def test_five_scalars_viscous_and_diffusive_against_the_oracle(gpu, oracle, name, phys, prob, dtype):
    """visc_coef and diff_coef > 0: one cell-centred diffusion solve per tracer (scalar_advance.f90:144-162), both diffusion types"""
    O, G = _one_level_pair(16, phys, prob, 5, 3, visc_coef=0.01, diff_coef=0.005, diffusion_type=dtype)
    _check_fields(O, G, name)
    G.close()


# ---- 2. passivity, bit for bit -----------------------------------------------------------------------------------------------------------------------
def _state(G, nsteps):
    dts = []
    for _ in range(nsteps):
        G.step()
        dts.append(G.dt)
    out = {"dt": np.array(dts)}
    nl = getattr(G, "nlev", 1)
    if nl > 1 or hasattr(G, "nregrids"):
        out["boxes"] = repr(G.boxes)
    for n in range(nl):
        for i in range(G.unew[n].nfabs()):
            for k, mf in (("u", G.unew[n]), ("s", G.snew[n]), ("gp", G.gp[n]), ("p", G.p[n])):
                out["%s%d_%d" % (k, n, i)] = mf.to_numpy(i)
    G.close()
    return out


def _passivity(make, nsteps, tracers=(1, 2, 3, 4, 5)):
    """make(fields) -> a driver whose tracer j (1-based) starts from tracer_value(fields[j - 1]).  The run with all tracers must equal, bit for bit,
    the nscal = 2 runs started from one of them: rho, u, gp, p, dt and the boxes from the first; tracer j from the j-th"""
    big = _state(make(tracers), nsteps)
    for j, f in enumerate(tracers):
        one = _state(make((f,)), nsteps)
        assert one.keys() == big.keys()
        assert np.array_equal(one["dt"], big["dt"]), (one["dt"], big["dt"])
        if "boxes" in one:
            assert one["boxes"] == big["boxes"]
        for k in one:
            if k in ("dt", "boxes"):
                continue
            if k.startswith("s"):
                assert_bits(big[k][..., [0, j + 1]], one[k], "%s: density and tracer %d (nscal = %d) against the nscal = 2 run" % (k, j + 1, len(tracers) + 1))
            elif j == 0:
                assert_bits(big[k], one[k], "%s (nscal = %d) against nscal = 2" % (k, len(tracers) + 1))


def _one_box_maker(n, decomp=(1, 1, 1), **kw):
    from varden_amd import driver

    def make(fields):
        ns = len(fields) + 1
        prm = params_for(WALLS, cflfac=0.9, nscal=ns, **kw)
        u0, s0 = driver.initdata_numpy((n,) * 3, [1.0 / n] * 3, 1, 3, ns)
        set_tracers(s0, (0, 0, 0), [1.0 / n] * 3, fields)
        return driver.Varden(n, WALLS, prm, init_shrink=0.1, init_iter=1, u0=u0, s0=s0, decomp=decomp)
    return make


@pytest.mark.parametrize("n,decomp,diff", [(64, (1, 1, 1), False), (64, (1, 1, 1), True), (256, (1, 1, 1), False), (64, (2, 2, 2), False), (64, (2, 2, 2), True)])
def test_tracers_are_passive_bit_for_bit_on_one_level(gpu, n, decomp, diff):
    """nscal = 6 against five nscal = 2 runs.  One box: the fused march with the update inside it (64^3; 256^3: several tiles and chunks per plane) and, with
    diffusion, the march without the update and one solve per tracer; eight boxes: the box-batched stage kernels"""
    kw = dict(visc_coef=0.001, diff_coef=0.001) if diff else {}
    _passivity(_one_box_maker(n, decomp, **kw), 2)


def test_tracers_are_passive_bit_for_bit_on_a_regridded_hierarchy(gpu):
    """a tagged two-level hierarchy on a 32^3 base, regrid_int = 2 (regrids at steps 1 and 3), diffusive: fillpatch, the copies between box lists, the composite
    diffusion solves, the edge restriction of the conservative flux -- every tracer as if alone"""
    from varden_amd import driver

    def make(fields):
        prm = lambda: params_for(WALLS, cflfac=0.9, nscal=len(fields) + 1, visc_coef=0.001, diff_coef=0.001)   # noqa: E731
        levels = driver.VardenAMR.tagged_grids(32, WALLS, prm(), max_levs=2, max_grid_size=16)
        return driver.VardenAMR(32, levels[0], WALLS, params=prm(), finer_levels=levels[1:], init_shrink=0.1, init_iter=1, do_initial_projection=1,
                                regrid_int=2, max_levs=2, max_grid_size=16, init_fn=init_with_tracers(fields))
    _passivity(make, 3)


def test_tracers_are_passive_bit_for_bit_in_2d(gpu):
    """dm = 2 (one box: k2_mkflux and the 2-D update, diffusive) and the extruded copy of a tagged 2-D hierarchy"""
    from varden_amd import driver
    from varden_amd.capi import default_params
    bc2 = [[15, 15], [15, 15]]

    def make2(fields):
        ns = len(fields) + 1
        prm = default_params(dm=2, cflfac=0.9, nscal=ns, visc_coef=0.001, diff_coef=0.001)
        u0, s0 = driver.initdata_numpy((64, 64), [1.0 / 64] * 2, 1, 3, ns, dm=2)
        set_tracers(s0, (0, 0, 0), [1.0 / 64] * 2 + [1.0], fields)
        return driver.Varden(64, [bc2[0], bc2[1], [0, 0]], prm, init_shrink=0.1, init_iter=1, u0=u0, s0=s0)
    _passivity(make2, 2)

    def make_ext(fields):
        prm = lambda: default_params(cflfac=0.9, nscal=len(fields) + 1, visc_coef=0.001)   # noqa: E731
        levels = driver.VardenAMR.tagged_grids((32, 32), bc2, prm(), max_levs=2, max_grid_size=32, extrude2d=8)
        init = init_with_tracers(fields, base=driver.extruded_initdata(1, len(fields) + 1))
        return driver.VardenAMR((32, 32), levels[0], bc2, params=prm(), finer_levels=levels[1:], extrude2d=8, init_shrink=0.1, init_iter=1,
                                do_initial_projection=1, init_fn=init)
    _passivity(make_ext, 2)


# ---- 3. hierarchies against the box-list oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_levs", [2, 3])
def test_four_scalars_on_a_tagged_hierarchy_against_the_box_list_oracle(gpu, oracle, max_levs):
    """nscal = 4, viscous and diffusive, on the boxes tagging makes of the bubble (tests/test_amr_gpu.py::test_tagged_hierarchy_against_the_box_list_oracle):
    start-up + two steps, dt bit for bit, equal FAC counts, every field to 1e-9 on every box of every level, composite mass of rho to round-off"""
    from varden_amd import advance as adv
    from varden_amd import driver
    vo = oracle
    nc, kw = 32, dict(cflfac=0.9, nscal=4, visc_coef=0.001, diff_coef=0.001)
    init = init_with_tracers(FIVE[:3])
    levels = driver.VardenAMR.tagged_grids(nc, WALLS, params_for(WALLS, **kw), max_levs=max_levs, max_grid_size=32)
    assert len(levels) == max_levs - 1
    G = driver.VardenAMR(nc, levels[0], WALLS, params=params_for(WALLS, **kw), finer_levels=levels[1:], init_shrink=0.1, init_iter=1, do_initial_projection=1, init_fn=init)
    O = vo.SimML(nc, levels, WALLS, prm=params_for(WALLS, **kw), init_shrink=0.1, init_iter=1, do_initial_projection=1, init_fn=init)
    assert G.initial_projection_stat[0] == O.initial_projection_stat[0]
    assert G.dt == O.dt

    def mass():
        m = 0.0
        for n in range(O.nlev):
            msk = O.levels[n].mask()
            if n + 1 < O.nlev:
                f = O.levels[n + 1]
                fm = f.mask()[::2, ::2, ::2]
                o = [f.lo[d] // 2 - O.levels[n].lo[d] for d in range(3)]
                cov = np.zeros_like(msk)
                cov[o[0]:o[0] + fm.shape[0], o[1]:o[1] + fm.shape[1], o[2]:o[2] + fm.shape[2]] = fm
                msk = msk & ~cov
            for i in range(G.sold[n].nfabs()):
                lo, hi = G.sold[n].get_box(i)
                sl = tuple(slice(lo[d] - O.levels[n].lo[d], hi[d] - O.levels[n].lo[d] + 1) for d in range(3))
                m += (G.sold[n].to_numpy(i)[3:-3, 3:-3, 3:-3, 0] * msk[sl]).sum() / 8.0 ** n
        return m
    m0 = mass()
    for step in range(2):
        O.step(); G.step()
        assert G.dt == O.dt, "dt diverged at step %d" % step
        cg = (adv.last_solver_stats("mac")[0], adv.last_solver_stats("hg")[0])
        assert cg == (O.mgstat[0].cycles, O.mgstat[1].cycles), "step %d: FAC iterations %r vs %r" % (step, cg, (O.mgstat[0].cycles, O.mgstat[1].cycles))
        for n in range(O.nlev):
            olo = O.levels[n].lo
            for nm, gm, om, g, tol in (("u", G.uold[n], O.uold[n], 3, 1e-9), ("s", G.sold[n], O.sold[n], 3, 1e-9), ("gp", G.gp[n], O.gp[n], 1, 1e-6)):
                for i in range(gm.nfabs()):
                    lo, hi = gm.get_box(i)
                    a = gm.to_numpy(i)[g:-g, g:-g, g:-g]
                    b = om.valid()[tuple(slice(lo[d] - olo[d], hi[d] - olo[d] + 1) for d in range(3))]
                    for c in range(b.shape[3]):
                        scale = max(float(np.abs(om.valid()[..., c]).max()), 1e-300)
                        err = float(np.abs(a[..., c] - b[..., c]).max())
                        assert err <= tol * scale, "level %d box %d step %d: %s[%d] differs by %.3e (scale %.3e)" % (n, i, step, nm, c, err, scale)
    m1 = mass()
    assert abs(m1 - m0) <= 1e-12 * m0, "composite mass drifted by %.3e" % ((m1 - m0) / m0)
    G.close()


# ---- 4. several ranks ----------------------------------------------------------------------------------------------------------------------------------
def _run_ranks(tmp_path, tag, nranks, mode):
    return launch_ranks("_tracers_worker.py", nranks, tmp_path, tag, (mode,), per_proc=2, agree=("dt", "nboxes", "nregrids"))      # two rank threads per process: at most two children


@pytest.mark.parametrize("mode", ["fixed", "tagged"])
def test_tracers_on_several_ranks_reproduce_one_rank(gpu, tmp_path, mode):
    """nscal = 5, viscous and diffusive, two and four ranks (two rank threads per process) through the RCCL test double: a fixed two-level hierarchy, and the tagged one with regrids"""
    ref = _run_ranks(tmp_path, mode + "1", 1, mode)
    if mode == "tagged":
        assert ref["nregrids"][0] >= 1
    for nr in (2, 4):
        got = _run_ranks(tmp_path, mode + str(nr), nr, mode)
        assert sorted(ref) == sorted(got)
        for k in sorted(ref):
            assert np.array_equal(ref[k], got[k]), "%d ranks: %s differs: max %.3e" % (nr, k, np.abs(ref[k] - got[k]).max())


# ---- 5. restart, plot files, inputs, Fortran -----------------------------------------------------------------------------------------------------------
def test_restart_and_plot_file_with_four_scalars(gpu, tmp_path):
    from varden_amd import driver, plotfile
    fine = [((8, 8, 8), (23, 23, 15)), ((8, 8, 16), (23, 23, 23))]
    prm = lambda: params_for(WALLS, cflfac=0.9, nscal=4, visc_coef=0.001, diff_coef=0.001)   # noqa: E731
    init = init_with_tracers(FIVE[:3])
    A = driver.VardenAMR(16, fine, WALLS, params=prm(), init_iter=1, do_initial_projection=1, init_fn=init)
    A.step()
    chk = plotfile.write_checkfile(A, base=str(tmp_path / "chk"))
    plt = plotfile.write_plotfile(A, base=str(tmp_path / "plt"))
    A.step(); A.step()
    ref = [A.uold[n].to_numpy(i) for n in range(A.nlev) for i in range(A.uold[n].nfabs())] + \
          [A.sold[n].to_numpy(i) for n in range(A.nlev) for i in range(A.sold[n].nfabs())]
    tA, dtA = A.time, A.dt
    A.close()
    c = plotfile.read_checkfile(chk)
    B = driver.VardenAMR(16, c["boxes"][1], WALLS, params=prm(), base_boxes=c["boxes"][0], restart=c, restart_step=1)
    B.step(); B.step()
    assert B.time == tA and B.dt == dtA
    got = [B.uold[n].to_numpy(i) for n in range(B.nlev) for i in range(B.uold[n].nfabs())] + \
          [B.sold[n].to_numpy(i) for n in range(B.nlev) for i in range(B.sold[n].nfabs())]
    for x, y in zip(ref, got):
        assert_bits(y, x, "state after restart, nscal = 4")
    B.close()
    p = plotfile.read_ml_multifab(plt)
    assert p["names"] == ["x_vel", "y_vel", "z_vel", "density", "tracer", "scalar_3", "scalar_4", "magvel", "vort", "gpx", "gpy", "gpz"]
    assert all(f.shape[3] == 2 * 3 + 4 + 2 for L in p["levels"] for f in L["fabs"])
    t4 = np.concatenate([f[..., 6].ravel() for f in p["levels"][0]["fabs"]])
    assert t4.min() > 0.05 and t4.max() < 0.95 and t4.std() > 0.01          # scalar_4 carries its own field


INPUTS4 = os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_3d_nscal4")      # the project's own inputs file, not one of the reference's (the others in that directory are)
MAIN = os.path.join(ROOT, "varden_amd", "fortran", "varden_main")


def test_inputs_with_four_scalars_python_and_fortran(gpu, tmp_path):
    """tests/golden/inputs/inputs_bubble_3d_nscal4 (nscal = 4, diffusive, two levels, regrid every second step): inputs.run writes plot files with the extra
    tracers, and the Fortran host varden_main runs the same file with the same boxes on every level and dt / time to 1e-12"""
    from varden_amd import inputs, plotfile
    rows = []

    def report(G):
        rows.append((G.istep, G.time, G.dt, G.nlev, [len(b) for b in G.boxes]))
    nl, G = inputs.run(open(INPUTS4).read(), report=report, outdir=str(tmp_path))
    assert int(nl["nscal"]) == 4 and G.nscal == 4 and G.istep == int(nl["max_step"]) and G.nregrids >= 1
    G.close()
    plts = sorted(d for d in os.listdir(str(tmp_path)) if d.startswith("plt"))
    assert plts, os.listdir(str(tmp_path))
    p = plotfile.read_ml_multifab(str(tmp_path / plts[-1]))
    assert p["names"][3:7] == ["density", "tracer", "scalar_3", "scalar_4"] and len(p["names"]) == 2 * 3 + 4 + 2
    if not os.path.exists(MAIN):
        if shutil.which("amdflang") is None and not os.path.exists("/opt/rocm/lib/llvm/bin/flang"):
            pytest.skip("no flang on this box and no prebuilt varden_main")
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(MAIN)])
    out = subprocess.run([MAIN, INPUTS4], cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    frows = []
    for ln in out.stdout.splitlines():
        m = re.match(r"\s*step\s+(\d+)\s+time\s+(\S+)\s+dt\s+(\S+)\s+\|u\|max\s+(\S+)\s+levels\s+(\d+)\s+boxes\s+(.*)", ln)
        if m:
            frows.append((int(m.group(1)), float(m.group(2)), float(m.group(3)), int(m.group(5)), [int(x) for x in m.group(6).split()]))
    assert len(frows) == len(rows), out.stdout[-3000:]
    for f, p_ in zip(frows, rows):
        assert f[0] == p_[0] and f[3] == p_[3] and f[4][:p_[3]] == p_[4], (f, p_)
        assert abs(f[1] - p_[1]) <= 1e-12 * p_[1] and abs(f[2] - p_[2]) <= 1e-12 * p_[2], (f, p_)
