"""The reference's own run-time inputs (exec/test/inputs_*, copied as data under tests/golden/inputs) through the path:
varden_amd/inputs.py parses the namelist and drives the start-up sequence, the time loop, tagging / regridding.  No reference
output exists to compare with (the regression plotfiles are not in the tree): the checks are the solver tolerances, finiteness, the
symmetries of the problems and the bookkeeping of the hierarchy."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INP = os.path.join(ROOT, "tests", "golden", "inputs")


def test_namelist_parser():
    from varden_amd import inputs
    d = inputs.parse_namelist(open(os.path.join(INP, "inputs_advect_3d")).read())
    assert d["dim_in"] == 3 and d["prob_type"] == 2 and d["max_levs"] == 3 and d["regrid_int"] == 2
    assert d["bcx_lo"] == 11 and d["bcx_hi"] == 12 and d["u_bc(1,1)"] == 1.0 and d["rho_bc(1,1)"] == 1.0
    assert d["visc_coef"] == 0.001 and d["grav"] == 0.0 and d["cluster_min_eff"] == 0.9
    d = inputs.parse_namelist(open(os.path.join(INP, "inputs_bubble_3d")).read())
    assert d["max_grid_size"] == 16 and d["init_shrink"] == 0.1 and d["grav"] == -9.8 and d["stop_time"] == 2.5


def level0(G, mf, comp):
    """valid data of level 0 assembled from its boxes (the inputs cut level 0 by max_grid_size)"""
    boxes = G.boxes[0] if isinstance(G.boxes[0][0][0], tuple) else G.boxes
    n = [max(b[1][d] for b in boxes) + 1 for d in range(3)]
    out = np.empty(n)
    g = mf.ng
    for i, (lo, hi) in enumerate(boxes):
        a = mf.to_numpy(i)
        out[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = a[g:a.shape[0] - g, g:a.shape[1] - g, g:a.shape[2] - g, comp]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,nsteps,nlev", [("inputs_bubble_3d", 8, 2), ("inputs_3d-regt", 4, 3), ("inputs_advect_3d", 4, 3), ("inputs_RayleighTaylor_3d", 5, 2)])
def test_reference_inputs_run(gpu, name, nsteps, nlev, tmp_path):
    from varden_amd import advance as adv
    from varden_amd import inputs
    text = open(os.path.join(INP, name)).read().replace("verbose = 1", "verbose = 0")
    seen = []

    def report(G):
        mac, hg = adv.last_solver_stats("mac"), adv.last_solver_stats("hg")
        assert mac[0] < 60 and hg[0] < 60, (G.istep, mac, hg)
        assert mac[2] <= 1e-10 * mac[1] or mac[1] == 0.0
        seen.append((G.istep, [len(b) for b in G.boxes], G.dt))

    nl, G = inputs.run(text, nsteps, report, outdir=str(tmp_path))
    assert G.nlev == nlev and G.istep == nsteps and G.nregrids >= (nsteps - 1) // 2
    assert os.path.isdir(str(tmp_path / "plt00000")) and G.files_written[0].endswith("plt00000")          # plot_int = 10: step 0 ...
    assert os.path.isdir(str(tmp_path / ("plt%05d" % nsteps)))                                            # ... and the last step (varden.f90:376)
    assert all(s[2] > 0 for s in seen)
    for n in range(G.nlev):
        for i in range(G.unew[n].nfabs()):
            assert np.isfinite(G.unew[n].to_numpy(i)).all() and np.isfinite(G.snew[n].to_numpy(i)).all()
    s0 = level0(G, G.snew[0], 0)
    if "Rayleigh" in name:                                    # periodic in x and y, heavy over light: the interface region stays within the two densities
        assert s0.min() >= 1.0 - 1e-3 and s0.max() <= 2.0 + 1e-3
        w = level0(G, G.unew[0], 2)
        assert np.abs(w).max() > 0.0
    elif "advect" not in name:                                # the bubble problems are mirror-symmetric in x and y ...
        # ... exactly so when the union of boxes is (two levels here); the clustered level 2 of the three-level case is not, and the
        # coarse-fine interfaces then sit at different places left and right: symmetric to truncation error only
        tol = 1e-8 if nlev == 2 else 1e-3
        assert np.abs(s0 - s0[::-1]).max() <= tol and np.abs(s0 - s0[:, ::-1]).max() <= tol
        w = level0(G, G.unew[0], 2)
        assert w.max() > 0.0                                   # the light bubble rises
    else:                                                     # inflow u = 1 at x-lo: the flow goes on in +x
        u = level0(G, G.unew[0], 0)
        assert u.mean() > 0.5
    G.close()


@pytest.mark.gpu
def test_vortextube_input_runs(gpu, tmp_path):
    """exec/test/inputs_vortextube_3d: one level, triply periodic, prob_type 4 (vortex tube), max_step = 1; the initial projection
    runs with the absolute tolerance hgproject.f90:125-127 gives this problem"""
    from varden_amd import advance as adv
    from varden_amd import inputs
    text = open(os.path.join(INP, "inputs_vortextube_3d")).read().replace("verbose = 1", "verbose = 0")
    nl, G = inputs.run(text, None, None, outdir=str(tmp_path))        # (plot_int = 1: the plot files go to the test's directory)
    assert G.istep == 1 and not hasattr(G, "nlev")
    u = G.unew[0].to_numpy()[3:-3, 3:-3, 3:-3]
    s = G.snew[0].to_numpy()[3:-3, 3:-3, 3:-3]
    assert np.isfinite(u).all() and np.isfinite(s).all()
    assert 0.9 < np.abs(u[..., 0]).max() < 1.1 and np.abs(s[..., 0] - 1.0).max() <= 1e-4           # the tube's axial velocity ~ 1; the corner-coupled conservative update keeps a constant density only to O(dt^2 grad u grad v) (mkflux.f90:1620-1626 vs 1874-1905), 1.3e-6 here
    assert adv.last_solver_stats("hg")[0] < 40
    G.close()


@pytest.mark.gpu
def test_checkpoint_and_restart_from_inputs(gpu, tmp_path):
    """inputs_bubble_3d with chk_int = 2: the run restarted from chk00002 (grids and state from the file, the regrid of step 3 included)
    ends in the same bits as the uninterrupted run; the plot file of step 4 lists the same boxes"""
    from varden_amd import inputs, plotfile
    text = open(os.path.join(INP, "inputs_bubble_3d")).read().replace("verbose = 1", "verbose = 0")
    text = text.replace("chk_int   = 100", "chk_int   = 2").replace("plot_int  = 10", "plot_int  = 4\n grids_file_name = 'grids.out'")
    assert "chk_int   = 2" in text and "plot_int  = 4" in text

    def valid(G):
        return [G.uold[n].to_numpy(i)[3:-3, 3:-3, 3:-3] for n in range(G.nlev) for i in range(G.uold[n].nfabs())] + \
               [G.p[n].to_numpy(i)[1:-1, 1:-1, 1:-1] for n in range(G.nlev) for i in range(G.p[n].nfabs())]

    nl, A = inputs.run(text, 4, None, outdir=str(tmp_path))
    names = [os.path.basename(f) for f in A.files_written]
    assert names == ["plt00000", "chk00000", "chk00002", "plt00004", "chk00004"], names
    ref, boxes, tA = valid(A), A.boxes, A.time
    grids = open(str(tmp_path / "grids.out")).read()
    assert grids.count("At step") == 1 + A.nregrids and ("   ((0, 0, 0) (31, 31, 31) (0,0,0))    8\n") in grids and "      ((16, 16, 16) (31, 31, 31) (0,0,0)) \n" in grids
    info = open(str(tmp_path / "plt00004" / "job_info")).read()
    assert "Grid Information" in info and "no slip wall" in info and "max_levs" in info
    A.close()
    nl, B = inputs.run(text.replace("&PROBIN", "&PROBIN\n restart = 2"), 4, None, outdir=str(tmp_path))
    assert B.istep == 4 and B.time == tA and B.boxes == boxes
    for x, y in zip(ref, valid(B)):
        assert np.array_equal(x, y)
    plt = plotfile.read_ml_multifab(str(tmp_path / "plt00004"))
    assert plt["nlevs"] == B.nlev and [L["boxes"] for L in plt["levels"]] == [list(b) for b in boxes]
    B.close()


@pytest.mark.gpu
def test_fixed_grids_reproduce_the_tagged_run(gpu, tmp_path):
    """the grids file a run writes (grids_file_name) read back as fixed_grids (src/initialize.f90:93-150): same boxes, same bits, with
    regridding switched off in both runs"""
    from varden_amd import inputs
    text = open(os.path.join(INP, "inputs_bubble_3d")).read().replace("verbose = 1", "verbose = 0")
    text = text.replace("regrid_int = 2", "regrid_int = -1").replace("plot_int  = 10", "plot_int  = 0").replace("chk_int   = 100", "chk_int   = 0")
    assert "regrid_int = -1" in text

    def valid(G):
        return [G.unew[n].to_numpy(i)[3:-3, 3:-3, 3:-3] for n in range(G.nlev) for i in range(G.unew[n].nfabs())]

    nl, A = inputs.run(text.replace("&PROBIN", "&PROBIN\n grids_file_name = 'grids.out'"), 3, None, outdir=str(tmp_path))
    ref, boxes = valid(A), A.boxes
    A.close()
    nl, B = inputs.run(text.replace("&PROBIN", "&PROBIN\n fixed_grids = 'grids.out'"), 3, None, outdir=str(tmp_path))
    assert B.boxes == boxes and B.nlev == 2
    for x, y in zip(ref, valid(B)):
        assert np.array_equal(x, y)
    B.close()


@pytest.mark.gpu
def test_the_restart_regression_case_of_the_reference(gpu, tmp_path):
    """Util/regression_testing/VARDEN-tests.ini [bubble-restart]: exec/test/inputs-restart-regt (three levels on a 64^3 base, regrid_int = 2, viscous, max_step = 8, chk_int = 4),
    restartFileNum = 4 -- the run continued from chk00004 must end where the uninterrupted run ends: the same boxes, time, dt and every field of every level BIT FOR BIT.
    (Until round 6 it did not: 3e-14 apart at step 8, and two runs of the uninterrupted case did not agree with each other either -- the two copies of a plane of MAC
    faces shared by two boxes differ by velpred's per-box dead band, and the edge restriction and the ghost-face exchange took whichever the scheduler wrote last;
    profiles/r06_determinism.txt.)"""
    from varden_amd import inputs
    text = open(os.path.join(INP, "inputs-restart-regt")).read().replace("verbose = 1", "verbose = 0").replace("mg_verbose = 1", "mg_verbose = 0")

    def valid(G):
        return [m.to_numpy(i)[g:-g, g:-g, g:-g] for mfs, g in ((G.uold, 3), (G.sold, 3), (G.gp, 1), (G.p, 1)) for n, m in enumerate(mfs) for i in range(m.nfabs())]
    nl, A = inputs.run(text, None, None, outdir=str(tmp_path))
    assert A.istep == 8 and A.nlev == 3 and "chk00004" in [os.path.basename(f) for f in A.files_written]
    ref, boxes, tA, dtA = valid(A), A.boxes, A.time, A.dt
    A.close()
    nl, B = inputs.run(text.replace("&PROBIN", "&PROBIN\n restart = 4"), None, None, outdir=str(tmp_path))
    assert B.istep == 8 and B.time == tA and B.dt == dtA and B.boxes == boxes
    for x, y in zip(ref, valid(B)):
        assert np.array_equal(x, y)
    B.close()


@pytest.mark.gpu
def test_three_level_regridding_run_is_reproducible_from_process_to_process(gpu):
    """inputs-restart-regt (three levels, max_grid_size 32, regrid_int = 2, viscous), eight steps, in three separate processes: the same bits after every step.  Until round 6
    such runs forked from step 6 on (differences of 1e-11; three to six variants in twelve runs): the two copies of a plane of MAC faces shared by two boxes differ by velpred's
    per-box dead band, and the edge restriction and the ghost-face exchange let the scheduler pick one (profiles/r06_determinism.txt)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for _ in range(3):
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "probes", "determinism_probe.py")], capture_output=True, text=True, timeout=300, cwd=root)
        assert r.returncode == 0, r.stderr[-1500:]
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith("inputs-restart-regt")][0])
    assert outs[0] == outs[1] == outs[2], outs
