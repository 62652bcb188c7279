"""Krylov bottom solvers of the two dm = 2 multigrids (vdn_params.mg_bottom_solver / hg_bottom_solver: 1 = BiCGStab, 2 = CG; csrc/dim2.hip on csrc/krylov_wg.h), after
tests/test_bottom_solver_gpu.py.  The solves are held against sparse DIRECT solutions of independently assembled systems (tests/assembled2d.py, itself held
against the oracle in tests/test_assembled_2d_cpu.py), with that file's bounds.

  (70, 66)  one coarsening, then 35 x 33 cells / 36 x 34 nodes: more points than the workgroup has threads -- the stride loops and a partial last stride
  (44, 52)  22 x 26 -> 11 x 13: three levels, unequal odd extents
  (24, 24)  ... -> 3 x 3 cells / 4 x 4 nodes: fewer unknowns than one wave
  (40, 12)  (20, 6) -> (10, 3): a bottom three cells wide
"""
import functools
import os

import numpy as np
import pytest

from tests import assembled2d as a2
from tests.children import launch_ranks
from tests.test_dim2_boxlists_gpu import BC2, Level2, ell_bc, params2, wrap
from tests.util import assert_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = a2.SHAPES
BCS = ["walls", "inout", "periodic", "periodic-x"]
ZERO = dict(calls=0, iters=0, max_iters=0, breakdowns=0)
MID = (44, 52)

cc_system = functools.lru_cache(maxsize=None)(a2.cc_system)        # computed once per (shape, boundary set), shared by the cases, never modified
nd_system = functools.lru_cache(maxsize=None)(a2.nd_system)


def test_the_boundary_sets_are_those_of_the_assembled_systems():
    for name in BCS:
        assert ell_bc(BC2[name])[:2] == a2.ELL2[name], name


def cuts2(n, parts):
    """box list of a 2-D domain of n[0] x n[1] cells: parts = (x widths, y widths)"""
    xs, ys = parts
    assert sum(xs) == n[0] and sum(ys) == n[1]
    boxes, y0 = [], 0
    for wy in ys:
        x0 = 0
        for wx in xs:
            boxes.append(((x0, y0, 0), (x0 + wx - 1, y0 + wy - 1, 0)))
            x0 += wx
        y0 += wy
    return boxes


class Level2R(Level2):
    """Level2 on n[0] x n[1] cells"""
    def __init__(self, n, boxes, phys):
        from varden_amd import boxlib as bl
        self.bl, self.n, self.boxes = bl, tuple(n), boxes
        self.pmask = [1 if phys[d][0] == -1 else 0 for d in range(2)] + [0]
        self.mla = bl.MLLayout([((0, 0, 0), (n[0] - 1, n[1] - 1, 0))], [boxes], pmask=self.pmask)
        self.mfs = []

    def gather(self, mf, ng, nodal=(0, 0, 0)):
        out = np.full((self.n[0] + nodal[0], self.n[1] + nodal[1], mf.nc), np.nan)
        for i, (lo, hi) in enumerate(self.boxes):
            a = mf.to_numpy(i)[:, :, 0, :]
            v = a[ng:a.shape[0] - ng, ng:a.shape[1] - ng] if ng else a
            out[lo[0]:lo[0] + v.shape[0], lo[1]:lo[1] + v.shape[1]] = v
        return out


def start(bcname, prm):
    from varden_amd import boxlib as bl
    bl.initialize(params2(BC2[bcname], **prm), 0, 1, 0)


def cc_solve_once(n, bcname, b=None, parts=None, with_alpha=False, **prm):
    """(alpha - div beta grad) phi = b from phi = 0 with homogeneous Dirichlet data, at rel 1e-11: phi on the cells, cycles, bottom statistics"""
    from varden_amd import advance as adv
    S = cc_system(n, bcname, with_alpha)
    start(bcname, prm)
    L = Level2R(n, cuts2(n, parts or ((n[0],), (n[1],))), BC2[bcname])
    gphi = L.scatter(np.zeros((n[0] + 2, n[1] + 2, 1)), 1)
    beta = [L.scatter(S["bx"][:, :, None], 0, (1, 0, 0)), L.scatter(S["by"][:, :, None], 0, (0, 1, 0))]
    alpha = L.scatter(S["alpha"][:, :, None], 0) if with_alpha else None
    cyc, r0, r = adv.cc_solve(L.scatter((S["b"] if b is None else b)[:, :, None], 0), gphi, beta, S["dx"], ell_bc(BC2[bcname]), 1e-11, alpha=alpha)
    x = L.gather(gphi, 1)[:, :, 0]
    st = adv.last_bottom_stats("mac")
    L.close()
    return x, cyc, st


def nd_solve_once(n, bcname, u=None, parts=None, **prm):
    """K phi = -D u from phi = 0 at rel 1e-12: phi on the nodes 0..n, cycles, bottom statistics"""
    from varden_amd import advance as adv
    S = nd_system(n, bcname)
    start(bcname, prm)
    L = Level2R(n, cuts2(n, parts or ((n[0],), (n[1],))), BC2[bcname])
    ug, sg = np.zeros((n[0] + 2, n[1] + 2, 2)), np.zeros((n[0] + 2, n[1] + 2, 1))       # periodic images in the ghost layer, zero beyond walls and outflow
    ug[1:-1, 1:-1] = S["u"] if u is None else u
    sg[1:-1, 1:-1, 0] = S["sig"]
    wrap(ug, 1, L.pmask); wrap(sg, 1, L.pmask)
    nodal = (1, 1, 0)
    gphi = L.scatter(np.zeros((n[0] + 3, n[1] + 3, 1)), 1, nodal)
    cyc, r0, r = adv.nd_solve(L.scatter(np.zeros((n[0] + 3, n[1] + 3, 1)), 1, nodal), gphi, L.scatter(sg, 1), L.scatter(ug, 1), S["dx"], ell_bc(BC2[bcname]), 1e-12)
    y = L.gather(gphi, 1, nodal)[:, :, 0]
    st = adv.last_bottom_stats("hg")
    L.close()
    return y, cyc, st


# the same systems with the default bottom sweeps: solved once per (shape, boundary set), shared by the two solver values
@functools.lru_cache(maxsize=None)
def cc_default(n, bcname, with_alpha=False):
    return cc_solve_once(n, bcname, with_alpha=with_alpha)


@functools.lru_cache(maxsize=None)
def nd_default(n, bcname):
    return nd_solve_once(n, bcname)


def check_cc(n, bcname, solver, with_alpha=False):
    S = cc_system(n, bcname, with_alpha)
    x, cyc, st = cc_solve_once(n, bcname, with_alpha=with_alpha, mg_bottom_solver=solver)
    x0, cyc0, st0 = cc_default(n, bcname, with_alpha)
    xm, b = x.ravel(order="F"), S["b"].ravel(order="F")
    res = np.abs(b - S["A"] @ xm).max() / np.abs(b).max()
    if S["singular"]:
        xm = xm - xm.mean()
    err = np.abs(xm - S["xd"]).max() / np.abs(S["xd"]).max()
    print("cc %s %s%s solver %d: %d cycles (bottom sweeps: %d), residual %.3e |b|, error %.3e, bottom %r" % (n, bcname, " alpha" if with_alpha else "", solver, cyc, cyc0, res, err, st))
    assert res <= 2e-11, "the HIP solution leaves %.3e |b| in the assembled system" % res
    assert err <= 1e-8, "%s: HIP multigrid (%d cycles) vs direct solution: %.3e" % (bcname, cyc, err)
    assert st["iters"] > 0 and st["calls"] > 0 and st["max_iters"] > 0 and st["breakdowns"] == 0, st
    assert st0 == ZERO, st0
    assert cyc <= cyc0 + 1, "Krylov bottom: %d V-cycles, bottom sweeps: %d" % (cyc, cyc0)


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("bcname", BCS)
@pytest.mark.parametrize("n", SHAPES)
def test_cc_solve_with_a_krylov_bottom_against_a_direct_solve(gpu, n, bcname, solver):
    check_cc(n, bcname, solver)


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("bcname", ["walls", "inout"])
def test_cc_solve_with_alpha_and_a_krylov_bottom_against_a_direct_solve(gpu, bcname, solver):
    """the solve of the viscous and diffusive steps: alpha a smooth positive cell field, the system regular whatever the faces"""
    check_cc(MID, bcname, solver, with_alpha=True)


def test_the_alpha_solve_in_three_dimensions_against_a_direct_solve(gpu):
    """advance.cc_solve(alpha=) is one entry for both dimensions: the same check on (12, 10, 8) cells (levels 12 x 10 x 8 and 6 x 5 x 4), default bottom, so
    that the dm = 3 side of the hook does not go untested"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    from tests.test_bottom_solver_gpu import cc_system as cc_system3, ell as ell3
    from tests.test_operators_assembled_cpu import smooth
    from tests.util import BC_SETS, Case
    from varden_amd import advance as adv
    n, bcname = (12, 10, 8), "inout"
    A, beta, b, _, _ = cc_system3(n, bcname)
    al = 40.0 * (2.0 + 0.45 * smooth(n, [1.0 / max(n)] * 3, 9))
    A = (A + sp.diags(al.ravel(order="F"))).tocsc()
    xd = spla.spsolve(A, b.ravel(order="F"))
    case = Case(n, BC_SETS[bcname], seed=3, iso=True)
    rh, phi, alpha = case.ofab(0, 1), case.ofab(1, 1), case.ofab(0, 1)
    rh.a[..., 0] = b
    alpha.a[..., 0] = al
    bf = [case.ofab(0, 1, tuple(1 if t == d else 0 for t in range(3))) for d in range(3)]
    for d in range(3):
        bf[d].a[..., 0] = beta[d]
    gphi = case.gmf(phi)
    cyc, r0, r = adv.cc_solve(case.gmf(rh), gphi, [case.gmf(x) for x in bf], case.dx, ell3(bcname), 1e-11, alpha=case.gmf(alpha))
    xm = gphi.to_numpy()[1:-1, 1:-1, 1:-1, 0].ravel(order="F")
    case.close()
    res = np.abs(b.ravel(order="F") - A @ xm).max() / np.abs(b).max()
    err = np.abs(xm - xd).max() / np.abs(xd).max()
    print("cc %s %s alpha, dm = 3: %d cycles, residual %.3e |b|, error %.3e" % (n, bcname, cyc, res, err))
    assert res <= 2e-11 and err <= 1e-8, (res, err)


@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("bcname", BCS)
@pytest.mark.parametrize("n", SHAPES)
def test_nd_solve_with_a_krylov_bottom_against_a_direct_solve(gpu, n, bcname, solver):
    S = nd_system(n, bcname)
    y, cyc, st = nd_solve_once(n, bcname, hg_bottom_solver=solver)
    y0, cyc0, st0 = nd_default(n, bcname)
    ym = S["NL"].from_grid(y)[S["free"]]
    if S["singular"]:
        ym = ym - ym.mean()
    err = np.abs(ym - S["yd"]).max() / np.abs(S["yd"]).max()
    print("nd %s %s solver %d: %d cycles (bottom sweeps: %d), error %.3e, bottom %r" % (n, bcname, solver, cyc, cyc0, err, st))
    assert err <= 1e-8, "%s: HIP nodal multigrid (%d cycles) vs direct solution: %.3e" % (bcname, cyc, err)
    assert st["iters"] > 0 and st["calls"] > 0 and st["max_iters"] > 0 and st["breakdowns"] == 0, st
    assert st0 == ZERO, st0
    assert cyc <= cyc0 + 1, "Krylov bottom: %d V-cycles, bottom sweeps: %d" % (cyc, cyc0)


def test_the_default_stays_the_default(gpu):
    """-1 (this library's default), 0 and 4 are all the bottom sweeps: bit-identical phi, no Krylov iteration"""
    xs, ys = [], []
    for solver in (-1, 0, 4):
        x, cyc, st = cc_solve_once(MID, "walls", mg_bottom_solver=solver, hg_bottom_solver=solver)
        assert st == ZERO, (solver, st)
        y, cyc, st = nd_solve_once(MID, "walls", mg_bottom_solver=solver, hg_bottom_solver=solver)
        assert st == ZERO, (solver, st)
        xs.append(x); ys.append(y)
    for q in (1, 2):
        assert_bits(xs[0], xs[q], "cell-centred phi, bottom solver -1 against %d" % (-1, 0, 4)[q])
        assert_bits(ys[0], ys[q], "nodal phi, bottom solver -1 against %d" % (-1, 0, 4)[q])


@pytest.mark.parametrize("solver", [1, 2])
def test_the_same_solve_twice_gives_the_same_bits(gpu, solver):
    x1, c1, s1 = cc_solve_once(MID, "inout", mg_bottom_solver=solver)
    x2, c2, s2 = cc_solve_once(MID, "inout", mg_bottom_solver=solver)
    assert_bits(x1, x2, "cell-centred phi of two identical solves")
    assert (c1, s1) == (c2, s2) and s1["iters"] > 0
    y1, c1, s1 = nd_solve_once(MID, "inout", hg_bottom_solver=solver)
    y2, c2, s2 = nd_solve_once(MID, "inout", hg_bottom_solver=solver)
    assert_bits(y1, y2, "nodal phi of two identical solves")
    assert (c1, s1) == (c2, s2) and s1["iters"] > 0


@pytest.mark.parametrize("solver", [1, 2])
def test_a_zero_right_hand_side_returns_zero(gpu, solver):
    x, cyc, st = cc_solve_once(MID, "walls", b=np.zeros(MID), mg_bottom_solver=solver)
    assert np.isfinite(x).all() and not x.any() and st["breakdowns"] == 0, st
    y, cyc, st = nd_solve_once(MID, "walls", u=np.zeros(MID + (2,)), hg_bottom_solver=solver)
    assert np.isfinite(y).all() and not y.any() and st["breakdowns"] == 0, st


@pytest.mark.parametrize("bcname", ["walls", "inout", "periodic"])
def test_krylov_bottoms_are_decomposition_blind(gpu, bcname):
    """CG bottoms on one box, on 2 x 2 boxes and on an unequal 32 + 12 cut: the solvers work on the gathered level, so phi comes out bit for bit the same, with
    the same cycles and the same bottom statistics"""
    prm = dict(mg_bottom_solver=2, hg_bottom_solver=2)
    xr, cr, sr = cc_solve_once(MID, bcname, **prm)
    yr, dr, tr = nd_solve_once(MID, bcname, **prm)
    assert sr["iters"] > 0 and tr["iters"] > 0 and np.isfinite(xr).all() and np.isfinite(yr).all()
    for parts in (((22, 22), (26, 26)), ((32, 12), (52,))):
        x, c, s = cc_solve_once(MID, bcname, parts=parts, **prm)
        assert (c, s) == (cr, sr), (parts, c, s, cr, sr)
        assert_bits(x, xr, "cell-centred phi on %r" % (parts,))
        y, d, t = nd_solve_once(MID, bcname, parts=parts, **prm)
        assert (d, t) == (dr, tr), (parts, d, t, dr, tr)
        assert_bits(y, yr, "nodal phi on %r" % (parts,))


# ---- whole steps ---------------------------------------------------------------------------------------------------------------------------
def run_steps(nsteps, **prm):
    from varden_amd import advance as adv
    from varden_amd import driver
    phys = BC2["walls"]
    G = driver.Varden((40, 40), [phys[0], phys[1], [0, 0]], params2(phys, cflfac=0.9, **prm), prob_type=1, init_shrink=0.1, init_iter=1)
    stats = []
    for _ in range(nsteps):
        G.step()
        stats.append((adv.last_bottom_stats("mac"), adv.last_bottom_stats("hg")))
    return G, stats


CG = dict(mg_bottom_solver=2, hg_bottom_solver=2)


@pytest.mark.parametrize("visc_coef,diff_coef", [(0.0, 0.0), (0.01, 0.005)])
def test_full_steps_with_cg_bottoms_match_the_default(gpu, visc_coef, diff_coef):
    """three steps of the bubble on 40^2 cells (bottom levels 5^2 cells / 6^2 nodes); visc_coef, diff_coef > 0: the viscous and diffusive solves take the alpha path"""
    A, st0 = run_steps(3, visc_coef=visc_coef, diff_coef=diff_coef)
    ref = dict(u=A.gather_valid(A.unew[0]), rho=A.gather_valid(A.snew[0])[..., 0])
    A.close()
    B, st = run_steps(3, visc_coef=visc_coef, diff_coef=diff_coef, **CG)
    got = dict(u=B.gather_valid(B.unew[0]), rho=B.gather_valid(B.snew[0])[..., 0])
    B.close()
    for nm in ("u", "rho"):
        scale = np.abs(ref[nm]).max()
        err = np.abs(got[nm] - ref[nm]).max()
        print("visc %g: %s differs by %.3e (scale %.3e)" % (visc_coef, nm, err, scale))
        assert scale > 0 and err <= 1e-9 * scale, "%s differs by %.3e (scale %.3e)" % (nm, err, scale)
    for mac, hg in st:
        assert mac["iters"] > 0 and hg["iters"] > 0 and mac["breakdowns"] == 0 and hg["breakdowns"] == 0, (mac, hg)
    for mac, hg in st0:
        assert mac == ZERO and hg == ZERO


def test_full_steps_with_cg_bottoms_match_the_oracle(gpu, oracle):
    """the oracle has no Krylov bottom: an independent solution of the same systems.  The bounds of tests/test_dim2_gpu.py: check_pair2"""
    from tests.test_dim2_gpu import check_pair2
    phys = BC2["walls"]
    O = oracle.Sim((40, 40), [phys[0], phys[1], [0, 0]], params2(phys, cflfac=0.9), prob_type=1, init_shrink=0.1, init_iter=1, dm=2)
    from varden_amd import advance as adv
    from varden_amd import driver
    G = driver.Varden((40, 40), [phys[0], phys[1], [0, 0]], params2(phys, cflfac=0.9, **CG), prob_type=1, init_shrink=0.1, init_iter=1)
    for _ in range(3):
        O.step(); G.step()
        mac, hg = adv.last_bottom_stats("mac"), adv.last_bottom_stats("hg")
        assert mac["iters"] > 0 and hg["iters"] > 0 and mac["breakdowns"] == 0 and hg["breakdowns"] == 0, (mac, hg)
        assert abs(G.dt - O.dt) <= 1e-9 * O.dt, (G.dt, O.dt)
    check_pair2(O, G, "bubble-walls-cg")
    G.close()


def test_the_2d_cg_inputs_file_runs(gpu, tmp_path):
    from varden_amd import advance as adv
    from varden_amd import inputs
    text = open(os.path.join(ROOT, "tests", "golden", "inputs", "inputs_bubble_2d_n40_cg")).read()
    nl, G = inputs.run(text, 3, None, outdir=str(tmp_path))
    assert G.dm == 2 and G.istep == 3 and len(G.boxes) == 1
    u, s = G.gather_valid(G.uold[0]), G.gather_valid(G.sold[0])
    mac, hg = adv.last_bottom_stats("mac"), adv.last_bottom_stats("hg")
    G.close()
    assert np.isfinite(u).all() and np.isfinite(s).all() and np.abs(u).max() > 0
    assert mac["iters"] > 0 and hg["iters"] > 0 and mac["breakdowns"] == 0 and hg["breakdowns"] == 0, (mac, hg)


# ---- several ranks -------------------------------------------------------------------------------------------------------------------------
def run_ranks(tmp_path, tag, nranks):
    return launch_ranks("_bottom_solver_2d_worker.py", nranks, tmp_path, tag, (), agree=("dt", "mac_iters", "hg_iters"), timeout=300, overlap=None)


def test_two_ranks_reproduce_one_rank_bits_with_cg_bottoms(gpu, tmp_path):
    """(44, 22) cells in two boxes of 22^2: every rank holds the gathered level and its bottom of 22 x 11 cells / 23 x 12 nodes, solved by CG on every rank; the
    reductions have a fixed order, so two ranks give the bits of one rank on the same two boxes"""
    ref = run_ranks(tmp_path, "ref", 1)
    got = run_ranks(tmp_path, "mr", 2)
    assert sorted(ref) == sorted(got)
    assert ref["mac_iters"].min() > 0 and ref["hg_iters"].min() > 0
    for k in sorted(ref):
        assert np.array_equal(ref[k], got[k]), "%s differs: max %.3e" % (k, np.abs(ref[k] - got[k]).max())
    assert np.isfinite(got["u0"]).all() and np.abs(got["u0"]).max() > 0
