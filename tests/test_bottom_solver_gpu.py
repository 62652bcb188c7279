"""Krylov bottom solvers of the two multigrids (vdn_params.mg_bottom_solver / hg_bottom_solver: 1 = BiCGStab, 2 = CG; csrc/krylov_wg.h) on the smallest shapes on
which each path can go wrong.  The solves are held against sparse DIRECT solutions of independently assembled systems (tests/assembled.py), exactly as
tests/test_operators_assembled_gpu.py holds the default bottom sweeps: the same tolerances, Case and smooth().

  (22, 22, 22)  one coarsening, then 11^3 cells / 12^3 nodes: more unknowns than the workgroup has threads, odd periodic extents; kk_bottom_krylov<LV>
  (22, 26, 30)  bottom 11 x 13 x 15: unequal extents
  (24, 24, 24)  6^3 and 3^3 cells (7^3 and 4^3 nodes) sit inside the tail-cycle kernel: kk_*_tailcycle<true>
  (40, 20, 12)  10 x 5 x 3: a small bottom outside the tail cycle
"""
import functools
import os

import numpy as np
import pytest

from tests import assembled as asm
from tests.children import launch_ranks
from tests.test_operators_assembled_cpu import smooth
from tests.test_operators_assembled_gpu import ELL_OF
from tests.util import BC_SETS, WALLS, Case, assert_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(22, 22, 22), (22, 26, 30), (24, 24, 24), (40, 20, 12)]
BCS = ["walls", "inout", "periodic"]


def ell(bcname):
    return [[ELL_OF[BC_SETS[bcname][d][s]] for s in range(2)] for d in range(3)]


# ---- the assembled systems and their direct solutions: computed once per (shape, boundary set), shared by the solver values, never modified ----
@functools.lru_cache(maxsize=None)
def cc_system(n, bcname):
    ellbc = ell(bcname)
    dx = [1.0 / max(n)] * 3
    rho = 2.0 + 0.45 * smooth(tuple(x + 2 for x in n), dx, 21, lo=(-1, -1, -1))
    for d in range(3):
        if ellbc[d][0] == asm.PER:                         # periodic images in the ghost layer
            sl_g, sl_s = [slice(None)] * 3, [slice(None)] * 3
            sl_g[d], sl_s[d] = 0, -2; rho[tuple(sl_g)] = rho[tuple(sl_s)]
            sl_g[d], sl_s[d] = -1, 1; rho[tuple(sl_g)] = rho[tuple(sl_s)]
    beta = []
    for d in range(3):                                    # mk_mac_coeffs (macproject.f90:376-394) in numpy
        hi_ = [slice(1, -1)] * 3; lo_ = [slice(1, -1)] * 3
        hi_[d] = slice(1, None); lo_[d] = slice(0, -1)
        beta.append(2.0 / (rho[tuple(hi_)] + rho[tuple(lo_)]))
    A = asm.cc_matrix(n, dx, beta, ellbc)
    rng = np.random.default_rng(5)
    b = smooth(n, dx, 7) + 0.1 * rng.standard_normal(n)
    singular = not any(ellbc[d][s] == asm.DIR for d in range(3) for s in range(2))
    if singular:
        b -= b.mean()
    xd, lam = asm.solve_maybe_singular(A, b.ravel(order="F"), np.ones(A.shape[0]) if singular else None)
    if singular:
        xd = xd - xd.mean()
    for a in beta + [b, xd]:
        a.setflags(write=False)
    return A, tuple(beta), b, xd, singular


def cc_solve_once(n, bcname, b, beta, **prm):
    from varden_amd import advance as adv
    case = Case(n, BC_SETS[bcname], seed=3, iso=True, **prm)
    rh, phi = case.ofab(0, 1), case.ofab(1, 1)
    rh.a[..., 0] = b
    bf = [case.ofab(0, 1, tuple(1 if t == d else 0 for t in range(3))) for d in range(3)]
    for d in range(3):
        bf[d].a[..., 0] = beta[d]
    gphi = case.gmf(phi)
    cyc, r0, r = adv.cc_solve(case.gmf(rh), gphi, [case.gmf(x) for x in bf], case.dx, ell(bcname), 1e-11)
    x = gphi.to_numpy()[1:-1, 1:-1, 1:-1, 0].copy()
    st = adv.last_bottom_stats("mac")
    case.close()
    return x, cyc, st


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("bcname", BCS)
@pytest.mark.parametrize("n", SHAPES)
def test_cc_solve_with_a_krylov_bottom_against_a_direct_solve(gpu, oracle, n, bcname, solver):
    A, beta, b, xd, singular = cc_system(n, bcname)
    x, cyc, st = cc_solve_once(n, bcname, b, beta, mg_bottom_solver=solver)
    x0, cyc0, st0 = cc_solve_once(n, bcname, b, beta)
    print("cc %s %s solver %d: %d cycles (bottom sweeps: %d), bottom %r" % (n, bcname, solver, cyc, cyc0, st))
    xm = x.ravel(order="F")
    res = b.ravel(order="F") - A @ xm
    assert np.abs(res).max() <= 2e-11 * np.abs(b).max(), "the HIP solution leaves %.3e |b| in the assembled system" % (np.abs(res).max() / np.abs(b).max())
    if singular:
        xm = xm - xm.mean()
    err = np.abs(xm - xd).max() / np.abs(xd).max()
    assert err <= 1e-8, "%s: HIP multigrid (%d cycles) vs direct solution: %.3e" % (bcname, cyc, err)
    assert st["iters"] > 0 and st["calls"] > 0 and st["max_iters"] > 0 and st["breakdowns"] == 0, st
    assert st0 == dict(calls=0, iters=0, max_iters=0, breakdowns=0), st0
    assert cyc <= cyc0 + 1, "Krylov bottom: %d V-cycles, bottom sweeps: %d" % (cyc, cyc0)


@functools.lru_cache(maxsize=None)
def nd_system(n, bcname):
    ellbc = ell(bcname)
    per = tuple(1 if BC_SETS[bcname][d][0] == -1 else 0 for d in range(3))
    dx = [1.0 / max(n)] * 3
    sig = 1.0 / (2.0 + 0.45 * smooth(n, dx, 5))
    u = np.stack([smooth(n, dx, 11 + c) for c in range(3)], axis=-1)
    NL = asm.NodalLevel(n, dx, per)
    K = NL.stiffness(sig) / NL.vol
    w = NL.load(u) / NL.vol
    dmask = NL.dirichlet_mask(ellbc)
    free = ~dmask
    singular = not dmask.any()
    yd, lam = asm.solve_maybe_singular(K[free][:, free], w[free], np.ones(int(free.sum())) if singular else None)
    if singular:
        yd = yd - yd.mean()
    for a in (sig, u, yd):
        a.setflags(write=False)
    return NL, sig, u, free, yd, singular


def nd_solve_once(oracle, n, bcname, sig_v, u_v, **prm):
    from varden_amd import advance as adv
    case = Case(n, BC_SETS[bcname], seed=4, iso=True, **prm)
    sig, u = case.ofab(1, 1), case.ofab(1, 3)
    sig.valid()[..., 0] = sig_v
    u.valid()[...] = u_v
    oracle.lib().vo_fill_boundary(sig.ref, case.opm)       # periodic images only; zero beyond walls / outflow (hg_multigrid.f90:73-79)
    oracle.lib().vo_fill_boundary(u.ref, case.opm)
    nodal = (1, 1, 1)
    grh, gphi = case.gmf(case.ofab(1, 1, nodal)), case.gmf(case.ofab(1, 1, nodal))
    cyc, r0, r = adv.nd_solve(grh, gphi, case.gmf(sig), case.gmf(u), case.dx, ell(bcname), 1e-12)
    y = gphi.to_numpy()[1:-1, 1:-1, 1:-1, 0].copy()
    st = adv.last_bottom_stats("hg")
    case.close()
    return y, cyc, st


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("bcname", BCS)
@pytest.mark.parametrize("n", SHAPES)
def test_nd_solve_with_a_krylov_bottom_against_a_direct_solve(gpu, oracle, n, bcname, solver):
    NL, sig, u, free, yd, singular = nd_system(n, bcname)
    y, cyc, st = nd_solve_once(oracle, n, bcname, sig, u, hg_bottom_solver=solver)
    y0, cyc0, st0 = nd_solve_once(oracle, n, bcname, sig, u)
    print("nd %s %s solver %d: %d cycles (bottom sweeps: %d), bottom %r" % (n, bcname, solver, cyc, cyc0, st))
    ym = NL.from_grid(y)[free]
    if singular:
        ym = ym - ym.mean()
    err = np.abs(ym - yd).max() / np.abs(yd).max()
    assert err <= 1e-8, "%s: HIP nodal multigrid (%d cycles) vs direct solution: %.3e" % (bcname, cyc, err)
    assert st["iters"] > 0 and st["calls"] > 0 and st["max_iters"] > 0 and st["breakdowns"] == 0, st
    assert st0 == dict(calls=0, iters=0, max_iters=0, breakdowns=0), st0
    assert cyc <= cyc0 + 1, "Krylov bottom: %d V-cycles, bottom sweeps: %d" % (cyc, cyc0)


def test_the_default_stays_the_default(gpu, oracle):
    """-1 (this library's default), 0 and 4 are all the bottom sweeps: bit-identical phi, no Krylov iteration"""
    n, bcname = (22, 22, 22), "walls"
    A, beta, b, xd, singular = cc_system(n, bcname)
    NL, sig, u, free, yd, singular = nd_system(n, bcname)
    xs, ys = [], []
    for solver in (-1, 0, 4):
        x, cyc, st = cc_solve_once(n, bcname, b, beta, mg_bottom_solver=solver, hg_bottom_solver=solver)
        assert st == dict(calls=0, iters=0, max_iters=0, breakdowns=0), (solver, st)
        y, cyc, st = nd_solve_once(oracle, n, bcname, sig, u, mg_bottom_solver=solver, hg_bottom_solver=solver)
        assert st == dict(calls=0, iters=0, max_iters=0, breakdowns=0), (solver, st)
        xs.append(x); ys.append(y)
    for q in (1, 2):
        assert_bits(xs[0], xs[q], "cell-centred phi, bottom solver -1 against %d" % (-1, 0, 4)[q])
        assert_bits(ys[0], ys[q], "nodal phi, bottom solver -1 against %d" % (-1, 0, 4)[q])


@pytest.mark.parametrize("solver", [1, 2])
def test_the_same_solve_twice_gives_the_same_bits(gpu, oracle, solver):
    n, bcname = (22, 22, 22), "inout"
    A, beta, b, xd, singular = cc_system(n, bcname)
    NL, sig, u, free, yd, singular = nd_system(n, bcname)
    x1, c1, s1 = cc_solve_once(n, bcname, b, beta, mg_bottom_solver=solver)
    x2, c2, s2 = cc_solve_once(n, bcname, b, beta, mg_bottom_solver=solver)
    assert_bits(x1, x2, "cell-centred phi of two identical solves")
    assert (c1, s1) == (c2, s2) and s1["iters"] > 0
    y1, c1, s1 = nd_solve_once(oracle, n, bcname, sig, u, hg_bottom_solver=solver)
    y2, c2, s2 = nd_solve_once(oracle, n, bcname, sig, u, hg_bottom_solver=solver)
    assert_bits(y1, y2, "nodal phi of two identical solves")
    assert (c1, s1) == (c2, s2) and s1["iters"] > 0


@pytest.mark.parametrize("solver", [1, 2])
def test_a_zero_right_hand_side_returns_zero(gpu, oracle, solver):
    n, bcname = (22, 22, 22), "walls"
    A, beta, b, xd, singular = cc_system(n, bcname)
    NL, sig, u, free, yd, singular = nd_system(n, bcname)
    x, cyc, st = cc_solve_once(n, bcname, np.zeros(n), beta, mg_bottom_solver=solver)
    assert np.isfinite(x).all() and not x.any() and st["breakdowns"] == 0, st
    y, cyc, st = nd_solve_once(oracle, n, bcname, sig, np.zeros(n + (3,)), hg_bottom_solver=solver)
    assert np.isfinite(y).all() and not y.any() and st["breakdowns"] == 0, st


def run_steps(nsteps, **prm):
    from varden_amd import advance as adv
    from varden_amd import driver
    from varden_amd.capi import default_params
    G = driver.Varden((20, 20, 20), WALLS, default_params(cflfac=0.9, **prm), prob_type=1, grav=-9.8, init_shrink=0.1, init_iter=1)
    stats = []
    for _ in range(nsteps):
        G.step()
        stats.append((adv.last_bottom_stats("mac"), adv.last_bottom_stats("hg")))
    out = dict(u=G.unew[0].to_numpy(0)[3:-3, 3:-3, 3:-3].copy(), rho=G.snew[0].to_numpy(0)[3:-3, 3:-3, 3:-3, 0].copy(), dt=G.dt)
    G.close()
    return out, stats


@pytest.mark.parametrize("visc_coef", [0.0, 0.001])
def test_full_steps_with_cg_bottoms_match_the_default(gpu, visc_coef):
    """three steps of the bubble on 20^3 cells (bottom levels 5^3 cells / 6^3 nodes); visc_coef > 0: the three viscous solves take the alpha path"""
    ref, st0 = run_steps(3, visc_coef=visc_coef)
    got, st = run_steps(3, visc_coef=visc_coef, mg_bottom_solver=2, hg_bottom_solver=2)
    for nm in ("u", "rho"):
        scale = np.abs(ref[nm]).max()
        err = np.abs(got[nm] - ref[nm]).max()
        print("visc %g: %s differs by %.3e (scale %.3e)" % (visc_coef, nm, err, scale))
        assert scale > 0 and err <= 1e-9 * scale, "%s differs by %.3e (scale %.3e)" % (nm, err, scale)
    for mac, hg in st:
        assert mac["iters"] > 0 and hg["iters"] > 0 and mac["breakdowns"] == 0 and hg["breakdowns"] == 0, (mac, hg)
    for mac, hg in st0:
        assert mac["iters"] == 0 and hg["iters"] == 0


def run_two_levels(nsteps, **prm):
    from varden_amd import driver
    from varden_amd.capi import default_params
    n = 24
    fine = [((n // 2,) * 3, (3 * n // 2 - 1,) * 3)]
    G = driver.VardenAMR(n, fine, WALLS, params=default_params(cflfac=0.9, **prm), prob_type=1, grav=-9.8, init_shrink=0.1, init_iter=1, do_initial_projection=1)
    for _ in range(nsteps):
        G.step()
    out = {}
    for lev in range(2):
        out["u%d" % lev] = G.unew[lev].to_numpy(0)[3:-3, 3:-3, 3:-3].copy()
        out["rho%d" % lev] = G.snew[lev].to_numpy(0)[3:-3, 3:-3, 3:-3, 0].copy()
    G.close()
    return out


def test_a_two_level_hierarchy_with_cg_bottoms_matches_the_default(gpu):
    """base 24^3 with one refined box: the level-0 cycles of the composite solves end in the tail-cycle kernel (6^3, 3^3 cells)"""
    ref = run_two_levels(2)
    got = run_two_levels(2, mg_bottom_solver=2, hg_bottom_solver=2)
    for nm in sorted(ref):
        scale = np.abs(ref[nm]).max()
        err = np.abs(got[nm] - ref[nm]).max()
        print("%s differs by %.3e (scale %.3e)" % (nm, err, scale))
        assert scale > 0 and err <= 1e-9 * scale, "%s differs by %.3e (scale %.3e)" % (nm, err, scale)


def run_ranks(tmp_path, tag, nranks):
    return launch_ranks("_bottom_solver_worker.py", nranks, tmp_path, tag, (), agree=("dt", "mac_iters", "hg_iters"), timeout=300)


def test_two_ranks_reproduce_one_rank_bits_with_cg_bottoms(gpu, tmp_path):
    """(44, 22, 22) in two boxes: the replicated tail is the single level 22 x 11 x 11, solved by CG on every rank; the reductions have a fixed order, so two
    ranks give the bits of one rank on the same two boxes"""
    ref = run_ranks(tmp_path, "ref", 1)
    got = run_ranks(tmp_path, "mr", 2)
    assert sorted(ref) == sorted(got)
    assert ref["mac_iters"].min() > 0 and ref["hg_iters"].min() > 0
    for k in sorted(ref):
        assert np.array_equal(ref[k], got[k]), "%s differs: max %.3e" % (k, np.abs(ref[k] - got[k]).max())
    assert np.isfinite(got["u0"]).all() and np.abs(got["u0"]).max() > 0
