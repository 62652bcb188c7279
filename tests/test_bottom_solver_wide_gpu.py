"""The Krylov bottom solvers over the whole GPU (csrc/krylov_grid.h): bottom levels of VDN_KRYLOV_GRID_MIN_POINTS points and more, where one workgroup
(csrc/krylov_wg.h, tests/test_bottom_solver_gpu.py) would stride over the level alone.

  (54, 50, 42)  one coarsening, then 27 x 25 x 21 cells / 28 x 26 x 22 nodes: three different odd extents, so rows and planes end inside a wave and inside a
                workgroup and the last workgroup is ragged (14175 cells = 55 workgroups of 256 and 95 cells; 16016 nodes = 62 and 144); with the periodic
                boundary set every direction stores node n as the image of node 0, counted once
  (34, 34, 34)  the smallest cube whose bottom (17^3 cells, 18^3 nodes) takes the grid-wide form: the full steps
  (68, 34, 34)  in two boxes of 34^3: the replicated tail is the single level 34 x 17 x 17

The systems are too large for a direct solve in a test's time, so the solutions are held by their residual in independently assembled matrices
(tests/assembled.py): the cell-centred ones at the bound of tests/test_bottom_solver_gpu.py, the nodal ones against what the solve with the bottom sweeps --
existing code, the reference here -- leaves in the same system."""
import functools
import os
import re

import numpy as np
import pytest

from tests import assembled as asm
from tests.children import launch_ranks
from tests.test_bottom_solver_gpu import ell, nd_solve_once
from tests.test_operators_assembled_cpu import smooth
from tests.util import BC_SETS, WALLS, Case, assert_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE = (54, 50, 42)
CUBE = 34
BCS = ["walls", "inout", "periodic"]
ZERO = dict(calls=0, iters=0, max_iters=0, breakdowns=0)


def crossover():
    txt = open(os.path.join(ROOT, "varden_amd", "csrc", "krylov_grid.h")).read()
    return int(re.search(r"#define\s+VDN_KRYLOV_GRID_MIN_POINTS\s+(\d+)", txt).group(1))


def test_the_shapes_sit_where_the_docstring_says():
    x = crossover()
    assert 22 * 11 * 11 < 23 * 12 * 12 < x, "the bottoms of tests/test_bottom_solver_gpu.py stay one workgroup"
    assert x <= 27 * 25 * 21 and x <= 17 ** 3 and x <= 34 * 17 * 17, "every bottom level of this file is grid-wide"
    assert (CUBE // 2 - 2) ** 3 < x <= (CUBE // 2) ** 3 and (CUBE // 2) % 2 == 1, "CUBE is the smallest cube whose bottom reaches the crossover"
    for m in (27, 25, 21, 17):
        assert m % 2 == 1


# ---- cell-centred -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cc_system(n, bcname, with_alpha):
    """tests/test_bottom_solver_gpu.py's system without its direct solve; with_alpha: the viscous / diffusive solves' cell coefficient"""
    ellbc = ell(bcname)
    dx = [1.0 / max(n)] * 3
    rho = 2.0 + 0.45 * smooth(tuple(x + 2 for x in n), dx, 21, lo=(-1, -1, -1))
    for d in range(3):
        if ellbc[d][0] == asm.PER:
            sl_g, sl_s = [slice(None)] * 3, [slice(None)] * 3
            sl_g[d], sl_s[d] = 0, -2; rho[tuple(sl_g)] = rho[tuple(sl_s)]
            sl_g[d], sl_s[d] = -1, 1; rho[tuple(sl_g)] = rho[tuple(sl_s)]
    beta = []
    for d in range(3):
        hi_ = [slice(1, -1)] * 3; lo_ = [slice(1, -1)] * 3
        hi_[d] = slice(1, None); lo_[d] = slice(0, -1)
        beta.append(2.0 / (rho[tuple(hi_)] + rho[tuple(lo_)]))
    al = 40.0 * (2.0 + 0.45 * smooth(n, dx, 9)) if with_alpha else None
    A = asm.cc_matrix(n, dx, beta, ellbc, alpha=al)
    rng = np.random.default_rng(5)
    b = smooth(n, dx, 7) + 0.1 * rng.standard_normal(n)
    singular = not with_alpha and not any(ellbc[d][s] == asm.DIR for d in range(3) for s in range(2))
    if singular:
        b -= b.mean()
    for a in beta + [b] + ([al] if with_alpha else []):
        a.setflags(write=False)
    return A, tuple(beta), b, al, singular


def cc_solve_once(n, bcname, b, beta, al=None, **prm):
    from varden_amd import advance as adv
    case = Case(n, BC_SETS[bcname], seed=3, iso=True, **prm)
    rh, phi = case.ofab(0, 1), case.ofab(1, 1)
    rh.a[..., 0] = b
    bf = [case.ofab(0, 1, tuple(1 if t == d else 0 for t in range(3))) for d in range(3)]
    for d in range(3):
        bf[d].a[..., 0] = beta[d]
    alpha = None
    if al is not None:
        alpha = case.ofab(0, 1)
        alpha.a[..., 0] = al
        alpha = case.gmf(alpha)
    gphi = case.gmf(phi)
    cyc, r0, r = adv.cc_solve(case.gmf(rh), gphi, [case.gmf(x) for x in bf], case.dx, ell(bcname), 1e-11, alpha=alpha)
    x = gphi.to_numpy()[1:-1, 1:-1, 1:-1, 0].copy()
    st, form = adv.last_bottom_stats("mac"), adv.last_bottom_form("mac")
    case.close()
    return x, cyc, st, form


@functools.lru_cache(maxsize=None)
def cc_default(n, bcname, with_alpha):
    A, beta, b, al, singular = cc_system(n, bcname, with_alpha)
    return cc_solve_once(n, bcname, b, beta, al)


@pytest.mark.parametrize("with_alpha", [False, True])
@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("bcname", BCS)
def test_cc_solve_with_a_grid_wide_bottom(gpu, oracle, bcname, solver, with_alpha):
    A, beta, b, al, singular = cc_system(WIDE, bcname, with_alpha)
    x, cyc, st, form = cc_solve_once(WIDE, bcname, b, beta, al, mg_bottom_solver=solver)
    x0, cyc0, st0, form0 = cc_default(WIDE, bcname, with_alpha)
    res = np.abs(b.ravel(order="F") - A @ x.ravel(order="F")).max() / np.abs(b).max()
    res0 = np.abs(b.ravel(order="F") - A @ x0.ravel(order="F")).max() / np.abs(b).max()
    print("cc %s %s%s solver %d: form %d, %d cycles (bottom sweeps: %d), residual %.3e |b| (bottom sweeps: %.3e), bottom %r"
          % (WIDE, bcname, " alpha" if with_alpha else "", solver, form, cyc, cyc0, res, res0, st))
    assert form == 2 and form0 == 0, (form, form0)
    assert st["iters"] > 0 and st["calls"] > 0 and st["max_iters"] > 0 and st["breakdowns"] == 0, st
    assert st0 == ZERO, st0
    assert res <= 2e-11, "the HIP solution leaves %.3e |b| in the assembled system" % res
    assert cyc <= cyc0 + 1, "Krylov bottom: %d V-cycles, bottom sweeps: %d" % (cyc, cyc0)


# ---- nodal ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nd_system(n, bcname):
    ellbc = ell(bcname)
    per = tuple(1 if BC_SETS[bcname][d][0] == -1 else 0 for d in range(3))
    dx = [1.0 / max(n)] * 3
    sig = 1.0 / (2.0 + 0.45 * smooth(n, dx, 5))
    u = np.stack([smooth(n, dx, 11 + c) for c in range(3)], axis=-1)
    NL = asm.NodalLevel(n, dx, per)
    free = ~NL.dirichlet_mask(ellbc)
    K = (NL.stiffness(sig) / NL.vol)[free][:, free].tocsr()
    w = (NL.load(u) / NL.vol)[free]
    for a in (sig, u, w):
        a.setflags(write=False)
    return NL, sig, u, free, K, w, bool(free.all())


def nd_residual(n, bcname, y):
    """max |w - K y| over the free nodes, relative to max |w|; singular systems: up to the constant the compatibility of w leaves free"""
    NL, sig, u, free, K, w, singular = nd_system(n, bcname)
    r = w - K @ NL.from_grid(y)[free]
    if singular:
        r = r - r.mean()
    return np.abs(r).max() / np.abs(w).max()


_ND_DEFAULT = {}


def nd_default(oracle, n, bcname):
    if (n, bcname) not in _ND_DEFAULT:
        NL, sig, u, free, K, w, singular = nd_system(n, bcname)
        _ND_DEFAULT[(n, bcname)] = nd_solve_once(oracle, n, bcname, sig, u)
    return _ND_DEFAULT[(n, bcname)]


def nd_solve_form(oracle, n, bcname, sig, u, **prm):
    from varden_amd import advance as adv
    y, cyc, st = nd_solve_once(oracle, n, bcname, sig, u, **prm)
    return y, cyc, st, adv.last_bottom_form("hg")


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("bcname", BCS)
def test_nd_solve_with_a_grid_wide_bottom(gpu, oracle, bcname, solver):
    NL, sig, u, free, K, w, singular = nd_system(WIDE, bcname)
    y, cyc, st, form = nd_solve_form(oracle, WIDE, bcname, sig, u, hg_bottom_solver=solver)
    y0, cyc0, st0 = nd_default(oracle, WIDE, bcname)
    res, res0 = nd_residual(WIDE, bcname, y), nd_residual(WIDE, bcname, y0)
    print("nd %s %s solver %d: form %d, %d cycles (bottom sweeps: %d), residual %.3e |w| (bottom sweeps: %.3e), bottom %r" % (WIDE, bcname, solver, form, cyc, cyc0, res, res0, st))
    assert form == 2, form
    assert st["iters"] > 0 and st["calls"] > 0 and st["max_iters"] > 0 and st["breakdowns"] == 0, st
    assert st0 == ZERO, st0
    assert np.isfinite(y).all() and res <= 2.0 * res0, "residual in the assembled system %.3e |w|; the solve with the bottom sweeps leaves %.3e" % (res, res0)
    assert cyc <= cyc0 + 1, "Krylov bottom: %d V-cycles, bottom sweeps: %d" % (cyc, cyc0)


# ---- bits, zero, the crossover ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", [1, 2])
def test_the_same_solve_in_two_fresh_layouts_gives_the_same_bits(gpu, oracle, solver):
    bcname = "inout"
    A, beta, b, al, singular = cc_system(WIDE, bcname, False)
    NL, sig, u, free, K, w, singular = nd_system(WIDE, bcname)
    x1, c1, s1, f1 = cc_solve_once(WIDE, bcname, b, beta, mg_bottom_solver=solver)
    x2, c2, s2, f2 = cc_solve_once(WIDE, bcname, b, beta, mg_bottom_solver=solver)
    assert_bits(x1, x2, "cell-centred phi of two identical solves")
    assert (c1, s1, f1) == (c2, s2, f2) and s1["iters"] > 0 and f1 == 2, (c1, s1, f1, c2, s2, f2)
    y1, c1, s1, f1 = nd_solve_form(oracle, WIDE, bcname, sig, u, hg_bottom_solver=solver)
    y2, c2, s2, f2 = nd_solve_form(oracle, WIDE, bcname, sig, u, hg_bottom_solver=solver)
    assert_bits(y1, y2, "nodal phi of two identical solves")
    assert (c1, s1, f1) == (c2, s2, f2) and s1["iters"] > 0 and f1 == 2, (c1, s1, f1, c2, s2, f2)


@pytest.mark.parametrize("solver", [1, 2])
def test_a_zero_right_hand_side_returns_zero(gpu, oracle, solver):
    bcname = "walls"
    A, beta, b, al, singular = cc_system(WIDE, bcname, False)
    NL, sig, u, free, K, w, singular = nd_system(WIDE, bcname)
    x, cyc, st, form = cc_solve_once(WIDE, bcname, np.zeros(WIDE), beta, mg_bottom_solver=solver)
    assert np.isfinite(x).all() and not x.any() and st["breakdowns"] == 0 and form == 2, (st, form)
    y, cyc, st, form = nd_solve_form(oracle, WIDE, bcname, sig, np.zeros(WIDE + (3,)), hg_bottom_solver=solver)
    assert np.isfinite(y).all() and not y.any() and st["breakdowns"] == 0 and form == 2, (st, form)


def test_below_the_crossover_nothing_changed(gpu, oracle):
    """(22, 22, 22): bottom 11^3 cells / 12^3 nodes -- CG in one workgroup reports form 1, the default reports form 0 and no statistics"""
    from tests.test_bottom_solver_gpu import cc_system as cc_small, nd_system as nd_small
    n, bcname = (22, 22, 22), "walls"
    A, beta, b, xd, singular = cc_small(n, bcname)
    NL, sig, u, free, yd, singular = nd_small(n, bcname)
    x, cyc, st, form = cc_solve_once(n, bcname, b, beta, mg_bottom_solver=2)
    assert form == 1 and st["iters"] > 0, (form, st)
    y, cyc, st, form = nd_solve_form(oracle, n, bcname, sig, u, hg_bottom_solver=2)
    assert form == 1 and st["iters"] > 0, (form, st)
    x, cyc, st, form = cc_solve_once(n, bcname, b, beta)
    assert form == 0 and st == ZERO, (form, st)
    y, cyc, st, form = nd_solve_form(oracle, n, bcname, sig, u)
    assert form == 0 and st == ZERO, (form, st)


# ---- full steps ----------------------------------------------------------------------------------------------------------------------------------------
INPUTS = """&PROBIN
 dim_in = 3
 prob_type = 1
 max_levs = 1
 n_cellx = %(n)d
 n_celly = %(n)d
 n_cellz = %(n)d
 max_grid_size = 64
 prob_hi_x = 1.0
 prob_hi_y = 1.0
 prob_hi_z = 1.0
 init_iter = 1
 do_initial_projection = 1
 max_step = 3
 plot_int = 0
 chk_int = 0
 stop_time = 2.5
 cflfac = 0.9
 init_shrink = 0.1
 visc_coef = %(visc)g
 diff_coef = 0.0
 grav = -9.8d0
 bcx_lo = 15
 bcx_hi = 15
 bcy_lo = 15
 bcy_hi = 15
 bcz_lo = 15
 bcz_hi = 15
 mg_bottom_solver = %(solver)d
 hg_bottom_solver = %(solver)d
 verbose = 0
 mg_verbose = 0
/
"""


def run_steps(how, tmp_path, visc_coef, solver):
    from varden_amd import advance as adv
    from varden_amd import driver, inputs
    from varden_amd.capi import default_params
    if how == "driver":
        G = driver.Varden((CUBE,) * 3, WALLS, default_params(cflfac=0.9, visc_coef=visc_coef, mg_bottom_solver=solver, hg_bottom_solver=solver),
                          prob_type=1, grav=-9.8, init_shrink=0.1, init_iter=1)
        for _ in range(3):
            G.step()
    else:
        nl, G = inputs.run(INPUTS % dict(n=CUBE, visc=visc_coef, solver=solver), 3, None, outdir=str(tmp_path))
        assert G.istep == 3 and (G.prm.mg_bottom_solver, G.prm.hg_bottom_solver) == (solver, solver)
    out = dict(u=G.unew[0].to_numpy(0)[3:-3, 3:-3, 3:-3].copy(), rho=G.snew[0].to_numpy(0)[3:-3, 3:-3, 3:-3, 0].copy())
    info = (adv.last_bottom_stats("mac"), adv.last_bottom_stats("hg"), adv.last_bottom_form("mac"), adv.last_bottom_form("hg"))
    G.close()
    return out, info


@pytest.mark.parametrize("how", ["driver", "inputs"])
@pytest.mark.parametrize("visc_coef", [0.0, 0.001])
def test_full_steps_with_grid_wide_cg_bottoms_match_the_default(gpu, tmp_path, visc_coef, how):
    """three steps of the bubble on 34^3 cells (bottom levels 17^3 cells / 18^3 nodes); visc_coef > 0: the three viscous solves of a step take the alpha path"""
    ref, (mac0, hg0, fm0, fh0) = run_steps(how, tmp_path, visc_coef, -1)
    got, (mac, hg, fm, fh) = run_steps(how, tmp_path, visc_coef, 2)
    for nm in ("u", "rho"):
        scale = np.abs(ref[nm]).max()
        err = np.abs(got[nm] - ref[nm]).max()
        print("%s, visc %g: %s differs by %.3e (scale %.3e)" % (how, visc_coef, nm, err, scale))
        assert scale > 0 and err <= 1e-9 * scale, "%s differs by %.3e (scale %.3e)" % (nm, err, scale)
    assert (fm, fh) == (2, 2) and (fm0, fh0) == (0, 0), (fm, fh, fm0, fh0)
    assert mac["iters"] > 0 and hg["iters"] > 0 and mac["breakdowns"] == 0 and hg["breakdowns"] == 0, (mac, hg)
    assert mac0 == ZERO and hg0 == ZERO


# ---- two ranks ------------------------------------------------------------------------------------------------------------------------------------------
def run_ranks(tmp_path, tag, nranks):
    return launch_ranks("_bottom_solver_wide_worker.py", nranks, tmp_path, tag, (), agree=("dt", "mac_iters", "hg_iters", "forms"), timeout=300)


def test_two_ranks_reproduce_one_rank_bits_with_grid_wide_cg_bottoms(gpu, tmp_path):
    """(68, 34, 34) in two boxes: the replicated tail is the single level 34 x 17 x 17 (35 x 18 x 18 nodes), solved grid-wide by CG on every rank with the same
    launch shape and the same order of sums: two ranks give the bits of one rank on the same two boxes"""
    ref = run_ranks(tmp_path, "ref", 1)
    got = run_ranks(tmp_path, "mr", 2)
    assert sorted(ref) == sorted(got)
    assert ref["mac_iters"].min() > 0 and ref["hg_iters"].min() > 0 and (ref["forms"] == 2).all(), ref["forms"]
    for k in sorted(ref):
        assert np.array_equal(ref[k], got[k]), "%s differs: max %.3e" % (k, np.abs(ref[k] - got[k]).max())
    assert np.isfinite(got["u0"]).all() and np.abs(got["u0"]).max() > 0
