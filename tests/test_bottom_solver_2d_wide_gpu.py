"""The Krylov bottom solvers of the two dm = 2 multigrids over the whole GPU (csrc/dim2.hip on csrc/krylov_grid.h): bottom levels of
VDN_KRYLOV_GRID_MIN_POINTS_2D points and more, where one workgroup (tests/test_bottom_solver_2d_gpu.py) would stride over the level alone.  The helpers and
bounds are that file's; the systems are those of tests/assembled2d.py, solved directly once per (shape, boundary set) and shared.

The crossover measured for the 5- and 9-point operators is 101^2 = 10201 points, not the 4913 of dm = 3 (the table is in krylov_grid.h), so the shapes are the
smallest of their kind above THAT constant, not (142, 150), (22, 902), (284, 300) and 150^2:

  WIDE2 (202, 206)  one coarsening, then 101 x 103 cells = 10403 / 102 x 104 nodes = 10608: two different odd extents, so rows end inside a wave and the last
                    workgroup is partial (10403 = 40 workgroups of 256 and 163 cells)
  STRIP (42, 974)   one coarsening, then 21 x 487 cells = 10227 / 22 x 488 nodes: a row far shorter than a wave, so t % n0 wraps three times per wave.  Its cap
                    is 12 x 487 iterations, launched in full by the first solve of a kind: CG only.  (Rows of 11 cells would need 929 of them and a cap of
                    11148: twice the launches.)  The nodal solves, and the cell-centred one with a Dirichlet face along the strip (inout)
  BAND  (90, 454)   one coarsening, then 45 x 227 cells = 10215: the cell-centred solves between Neumann ends (walls, periodic-x: the cell fill is 2 x 227
                    entries), rows still shorter than a wave.  Not STRIP, because of the arithmetic of the CHECK, not of the solver: check_cc evaluates b - A x
                    with the assembled matrix in double precision, and one such evaluation carries eps (|A| |x|) of round-off, which grows with the square of
                    the strip's length in cells and with |x| (largest between Neumann ends).  Computed from the assembled systems and their direct solutions
                    alone: 6.6e-11 |b| on STRIP for walls and periodic-x -- three times the bound of 2e-11 |b|, and the direct solution itself leaves 1.06e-10
                    |b| there -- against 8e-13 |b| on STRIP with inout, 7.4e-12 on (82, 498) and 4.1e-12 on BAND, a fifth of the bound
  DEEP  (404, 412)  two coarsenings, to WIDE2's bottom: the restriction and prolongation around a grid-wide bottom
  MID   (44, 52)    bottom 11 x 13: below the crossover, one workgroup as before
  202^2             the whole steps and the inputs file: bottom 101^2 cells / 102^2 nodes
  (284, 150)        the two ranks: bottom 142 x 75 cells = 10650 / 143 x 76 nodes
"""
import os
import re

import numpy as np
import pytest

from tests.children import launch_ranks
from tests.test_bottom_solver_2d_gpu import BCS, MID, ZERO, cc_solve_once, cc_system, nd_solve_once, nd_system
from tests.test_dim2_boxlists_gpu import BC2, params2
from tests.util import assert_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE2 = (202, 206)
STRIP = (42, 974)
BAND = (90, 454)
DEEP = (404, 412)
CG = dict(mg_bottom_solver=2, hg_bottom_solver=2)


def crossover():
    txt = open(os.path.join(ROOT, "varden_amd", "csrc", "krylov_grid.h")).read()
    return int(re.search(r"#define\s+VDN_KRYLOV_GRID_MIN_POINTS_2D\s+(\d+)", txt).group(1))


def test_the_shapes_sit_where_the_docstring_says():
    x = crossover()
    assert 11 * 13 < 12 * 14 < 22 * 11 < 23 * 12 < x, "MID and the bottoms of tests/test_bottom_solver_2d_gpu.py stay one workgroup"
    assert x <= 45 * 227 <= 21 * 487 < 101 * 103 and x <= 22 * 488 and x <= 102 * 104 and x <= 101 * 101 and x <= 142 * 75, "the bottoms of WIDE2, STRIP, BAND, DEEP, 202^2 and (284, 150) are grid-wide"
    for n, times in ((WIDE2, 1), (STRIP, 1), (BAND, 1), (DEEP, 2)):
        for m in n:
            assert m % (1 << times) == 0 and (m >> times) % 2 == 1, (n, times)
    assert tuple(m // 2 for m in DEEP) == WIDE2


def cc_form(n, bcname, **kw):
    from varden_amd import advance as adv
    x, cyc, st = cc_solve_once(n, bcname, **kw)
    return x, cyc, st, adv.last_bottom_form("mac")


def nd_form(n, bcname, **kw):
    from varden_amd import advance as adv
    y, cyc, st = nd_solve_once(n, bcname, **kw)
    return y, cyc, st, adv.last_bottom_form("hg")


def check_cc(n, bcname, solver, with_alpha=False):
    """tests/test_bottom_solver_2d_gpu.py::check_cc's bounds, and the form"""
    S = cc_system(n, bcname, with_alpha)
    x, cyc, st, form = cc_form(n, bcname, with_alpha=with_alpha, mg_bottom_solver=solver)
    xm, b = x.ravel(order="F"), S["b"].ravel(order="F")
    res = np.abs(b - S["A"] @ xm).max() / np.abs(b).max()
    if S["singular"]:
        xm = xm - xm.mean()
    err = np.abs(xm - S["xd"]).max() / np.abs(S["xd"]).max()
    print("cc %s %s%s solver %d: form %d, %d cycles, residual %.3e |b|, error %.3e, bottom %r" % (n, bcname, " alpha" if with_alpha else "", solver, form, cyc, res, err, st))
    assert form == 2, form
    assert res <= 2e-11, "the HIP solution leaves %.3e |b| in the assembled system" % res
    assert err <= 1e-8, "%s: HIP multigrid (%d cycles) vs direct solution: %.3e" % (bcname, cyc, err)
    assert st["iters"] > 0 and st["calls"] > 0 and st["max_iters"] > 0 and st["breakdowns"] == 0, st


def check_nd(n, bcname, solver):
    """the bounds of tests/test_bottom_solver_2d_gpu.py::test_nd_solve_with_a_krylov_bottom_against_a_direct_solve, and the form"""
    S = nd_system(n, bcname)
    y, cyc, st, form = nd_form(n, bcname, hg_bottom_solver=solver)
    ym = S["NL"].from_grid(y)[S["free"]]
    if S["singular"]:
        ym = ym - ym.mean()
    err = np.abs(ym - S["yd"]).max() / np.abs(S["yd"]).max()
    print("nd %s %s solver %d: form %d, %d cycles, error %.3e, bottom %r" % (n, bcname, solver, form, cyc, err, st))
    assert form == 2, form
    assert err <= 1e-8, "%s: HIP nodal multigrid (%d cycles) vs direct solution: %.3e" % (bcname, cyc, err)
    assert st["iters"] > 0 and st["calls"] > 0 and st["max_iters"] > 0 and st["breakdowns"] == 0, st


@pytest.mark.parametrize("with_alpha", [False, True])
@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("bcname", BCS)
def test_cc_solve_with_a_grid_wide_bottom_against_a_direct_solve(gpu, bcname, solver, with_alpha):
    check_cc(WIDE2, bcname, solver, with_alpha)


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("bcname", BCS)
def test_nd_solve_with_a_grid_wide_bottom_against_a_direct_solve(gpu, bcname, solver):
    check_nd(WIDE2, bcname, solver)


@pytest.mark.parametrize("n,bcname", [(BAND, "walls"), (BAND, "periodic-x"), (STRIP, "inout")])
def test_cc_solve_on_a_strip_with_rows_shorter_than_a_wave(gpu, n, bcname):
    """check_cc's bounds on strips where the round-off of its own residual evaluation stays below a fifth of its bound (the file's docstring)"""
    check_cc(n, bcname, 2)


@pytest.mark.parametrize("bcname", ["walls", "periodic-x"])
def test_nd_solve_on_a_strip_with_rows_shorter_than_a_wave(gpu, bcname):
    check_nd(STRIP, bcname, 2)


@pytest.mark.parametrize("bcname", ["walls", "inout"])
def test_three_levels_around_a_grid_wide_bottom(gpu, bcname):
    check_cc(DEEP, bcname, 2)
    check_nd(DEEP, bcname, 2)


def test_below_the_crossover_nothing_changed(gpu):
    """MID: CG in one workgroup reports form 1, the default reports form 0 and no statistics"""
    x, cyc, st, form = cc_form(MID, "walls", mg_bottom_solver=2)
    assert form == 1 and st["iters"] > 0, (form, st)
    y, cyc, st, form = nd_form(MID, "walls", hg_bottom_solver=2)
    assert form == 1 and st["iters"] > 0, (form, st)
    x, cyc, st, form = cc_form(MID, "walls")
    assert form == 0 and st == ZERO, (form, st)
    y, cyc, st, form = nd_form(MID, "walls")
    assert form == 0 and st == ZERO, (form, st)


@pytest.mark.parametrize("solver", [1, 2])
def test_the_same_solve_twice_gives_the_same_bits(gpu, solver):
    """the first solve of a kind launches the cap, the next one the budget derived from it: the same bits and statistics either way"""
    x1, c1, s1, f1 = cc_form(WIDE2, "inout", mg_bottom_solver=solver)
    x2, c2, s2, f2 = cc_form(WIDE2, "inout", mg_bottom_solver=solver)
    assert_bits(x1, x2, "cell-centred phi of two identical solves")
    assert (c1, s1, f1) == (c2, s2, f2) and s1["iters"] > 0 and f1 == 2, (c1, s1, f1, c2, s2, f2)
    y1, c1, s1, f1 = nd_form(WIDE2, "inout", hg_bottom_solver=solver)
    y2, c2, s2, f2 = nd_form(WIDE2, "inout", hg_bottom_solver=solver)
    assert_bits(y1, y2, "nodal phi of two identical solves")
    assert (c1, s1, f1) == (c2, s2, f2) and s1["iters"] > 0 and f1 == 2, (c1, s1, f1, c2, s2, f2)


@pytest.mark.parametrize("solver", [1, 2])
def test_a_zero_right_hand_side_returns_zero(gpu, solver):
    x, cyc, st, form = cc_form(WIDE2, "walls", b=np.zeros(WIDE2), mg_bottom_solver=solver)
    assert np.isfinite(x).all() and not x.any() and st["breakdowns"] == 0 and form == 2, (st, form)
    y, cyc, st, form = nd_form(WIDE2, "walls", u=np.zeros(WIDE2 + (2,)), hg_bottom_solver=solver)
    assert np.isfinite(y).all() and not y.any() and st["breakdowns"] == 0 and form == 2, (st, form)


@pytest.mark.parametrize("bcname", ["walls", "periodic"])
def test_grid_wide_bottoms_are_decomposition_blind(gpu, bcname):
    """CG bottoms on one box, on 2 x 2 equal boxes and on an unequal 140 + 62 cut: the solvers work on the gathered level and the launch shape comes from its
    point count alone, so phi comes out bit for bit the same, with the same cycles and the same bottom statistics"""
    xr, cr, sr, fr = cc_form(WIDE2, bcname, **CG)
    yr, dr, tr, gr = nd_form(WIDE2, bcname, **CG)
    assert sr["iters"] > 0 and tr["iters"] > 0 and np.isfinite(xr).all() and np.isfinite(yr).all() and (fr, gr) == (2, 2)
    for parts in (((101, 101), (103, 103)), ((140, 62), (206,))):
        x, c, s, f = cc_form(WIDE2, bcname, parts=parts, **CG)
        assert (c, s, f) == (cr, sr, 2), (parts, c, s, f, cr, sr)
        assert_bits(x, xr, "cell-centred phi on %r" % (parts,))
        y, d, t, g = nd_form(WIDE2, bcname, parts=parts, **CG)
        assert (d, t, g) == (dr, tr, 2), (parts, d, t, g, dr, tr)
        assert_bits(y, yr, "nodal phi on %r" % (parts,))


# ---- whole steps ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("visc_coef,diff_coef", [(0.0, 0.0), (0.01, 0.005)])
def test_full_steps_with_grid_wide_cg_bottoms_match_the_oracle(gpu, oracle, visc_coef, diff_coef):
    """one step (after the initial projection and the initial pressure iteration) of the bubble on 202^2 cells (bottom levels 101^2 cells / 102^2 nodes); visc_coef,
    diff_coef > 0: the viscous and diffusive solves take the alpha path.  The oracle has no Krylov bottom: an independent solution of the same systems.  The
    bounds of tests/test_dim2_gpu.py: check_pair2.  (One step, not the three of the 40^2 test: the oracle's bottom visit is 10201 sweeps of 101^2 cells, some
    twenty seconds of CPU work per step and as much again for its initialisation.)"""
    from tests.test_dim2_gpu import check_pair2
    from varden_amd import advance as adv
    from varden_amd import driver
    phys = BC2["walls"]
    kw = dict(cflfac=0.9, visc_coef=visc_coef, diff_coef=diff_coef)
    O = oracle.Sim((202, 202), [phys[0], phys[1], [0, 0]], params2(phys, **kw), prob_type=1, init_shrink=0.1, init_iter=1, dm=2)
    G = driver.Varden((202, 202), [phys[0], phys[1], [0, 0]], params2(phys, **kw, **CG), prob_type=1, init_shrink=0.1, init_iter=1)
    for _ in range(1):
        O.step(); G.step()
        mac, hg = adv.last_bottom_stats("mac"), adv.last_bottom_stats("hg")
        assert (adv.last_bottom_form("mac"), adv.last_bottom_form("hg")) == (2, 2)
        assert mac["iters"] > 0 and hg["iters"] > 0 and mac["breakdowns"] == 0 and hg["breakdowns"] == 0, (mac, hg)
        assert abs(G.dt - O.dt) <= 1e-9 * O.dt, (G.dt, O.dt)
    check_pair2(O, G, "bubble-walls-202-cg")
    G.close()


def test_the_2d_n202_cg_inputs_file_runs(gpu, tmp_path):
    from varden_amd import advance as adv
    from varden_amd import inputs
    text = open(os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_2d_n202_cg")).read()
    nl, G = inputs.run(text, 3, None, outdir=str(tmp_path))
    assert G.dm == 2 and G.istep == 3 and len(G.boxes) == 1
    u, s = G.gather_valid(G.uold[0]), G.gather_valid(G.sold[0])
    mac, hg = adv.last_bottom_stats("mac"), adv.last_bottom_stats("hg")
    forms = (adv.last_bottom_form("mac"), adv.last_bottom_form("hg"))
    G.close()
    assert np.isfinite(u).all() and np.isfinite(s).all() and np.abs(u).max() > 0
    assert forms == (2, 2), forms
    assert mac["iters"] > 0 and hg["iters"] > 0 and mac["breakdowns"] == 0 and hg["breakdowns"] == 0, (mac, hg)


# ---- several ranks -------------------------------------------------------------------------------------------------------------------------
def run_ranks(tmp_path, tag, nranks):
    return launch_ranks("_bottom_solver_2d_wide_worker.py", nranks, tmp_path, tag, (), agree=("dt", "mac_iters", "hg_iters", "forms"), timeout=300, overlap=None)


def test_two_ranks_reproduce_one_rank_bits_with_grid_wide_cg_bottoms(gpu, tmp_path):
    """(284, 150) cells in two boxes of 142 x 150: every rank holds the gathered level and its bottom of 142 x 75 cells / 143 x 76 nodes, solved grid-wide by CG on
    every rank with the same launch shape and the same order of sums: two ranks give the bits of one rank on the same two boxes"""
    ref = run_ranks(tmp_path, "ref", 1)
    got = run_ranks(tmp_path, "mr", 2)
    assert sorted(ref) == sorted(got)
    assert ref["mac_iters"].min() > 0 and ref["hg_iters"].min() > 0 and (ref["forms"] == 2).all(), ref["forms"]
    for k in sorted(ref):
        assert np.array_equal(ref[k], got[k]), "%s differs: max %.3e" % (k, np.abs(ref[k] - got[k]).max())
    assert np.isfinite(got["u0"]).all() and np.abs(got["u0"]).max() > 0
