"""tests/assembled2d.py (the yardstick of tests/test_bottom_solver_2d_gpu.py) held against the oracle's dm = 2 operators and solvers, without the library:
the five-point matrix against a hand-written one and against vo_cc_apply, the element-assembled Q1 matrix against the operator of the oracle's nodal
solver, and the sparse direct solutions against vo_cc_solve / vo_nd_solve (the algorithm of dim2.hip with sweeps at the bottom) at the shapes and boundary
sets of the GPU file, within its bounds.

vo_nd_apply, the oracle's test hook for K x, is written for dm = 3 fabs only.  The nodal operator is therefore reached through vo_nd_solve itself: with no
pre-smoothing sweep and max_iter = 0 it loads phi = x and b = -rh, takes ONE residual max |b - K x| over the free nodes and returns it; with
rh = -(K_assembled x) that residual IS max |K_assembled x - K_oracle x|."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import voracle as vo
from tests import assembled2d as a2
from varden_amd.capi import default_params

BCS = list(a2.ELL2)
cc_system = functools.lru_cache(maxsize=None)(a2.cc_system)
nd_system = functools.lru_cache(maxsize=None)(a2.nd_system)


def ell3(ell2):
    a = ((C.c_int * 2) * 3)()
    for d in range(2):
        for s in range(2):
            a[d][s] = ell2[d][s]
    return a


def box(n):
    return (0, 0, 0), (n[0] - 1, n[1] - 1, 0)


def beta_fabs(n, S):
    lo, hi = box(n)
    beta = [vo.Fab(lo, hi, 0, 1, (1, 0, 0), dm=2), vo.Fab(lo, hi, 0, 1, (0, 1, 0), dm=2), vo.Fab(lo, hi, 0, 1, dm=2)]      # (the third is never read)
    beta[0].a[:, :, 0, 0] = S["bx"]; beta[1].a[:, :, 0, 0] = S["by"]
    return beta


def test_the_five_point_matrix_is_cc_matrix_with_one_plane():
    """asm.cc_matrix on (n0, n1, 1) cells with Neumann z-faces against the matrix written out cell by cell, alpha included"""
    n = (12, 10)
    for bcname in BCS:
        dx, bx, by, b, alpha, singular = a2.cc_data(n, a2.ELL2[bcname], with_alpha=True)
        for al in (None, alpha):
            A = a2.cc_matrix5(n, dx, bx, by, a2.ELL2[bcname], al).toarray()
            B = a2.five_point(n, dx, bx, by, a2.ELL2[bcname], al)
            assert np.abs(A - B).max() <= 4e-16 * np.abs(B).max(), (bcname, np.abs(A - B).max() / np.abs(B).max())


@pytest.mark.parametrize("bcname", BCS)
@pytest.mark.parametrize("n", a2.SHAPES)
def test_cell_centred_operator_and_solution_2d(n, bcname):
    L = vo.lib()
    S = cc_system(n, bcname)
    lo, hi = box(n)
    beta = beta_fabs(n, S)
    dx3 = vo.dvec(S["dx"] + [1.0])
    x = np.random.default_rng(1).standard_normal(n)
    phi, out = vo.Fab(lo, hi, 1, 1, dm=2), vo.Fab(lo, hi, 0, 1, dm=2)
    phi.valid()[:, :, 0, 0] = x
    L.vo_cc_apply(phi.ref, None, vo.fab_ptr_array(beta), dx3, ell3(S["ell2"]), out.ref)
    Ax = (S["A"] @ x.ravel(order="F")).reshape(n, order="F")
    err = np.abs(out.a[:, :, 0, 0] - Ax).max()
    assert err <= 1e-13 * np.abs(Ax).max(), "oracle A x differs from the assembled matrix by %.3e (scale %.3e)" % (err, np.abs(Ax).max())
    rh = vo.Fab(lo, hi, 0, 1, dm=2); rh.a[:, :, 0, 0] = S["b"]
    phi.a[...] = 0.0
    st = vo.CMgStat()
    rc = L.vo_cc_solve(rh.ref, phi.ref, vo.fab_ptr_array(beta), dx3, ell3(S["ell2"]), C.c_double(1e-11), C.c_double(-1.0), 100, 2, 2, 8, 1, C.byref(st))
    assert rc == 0, st.cycles
    xm = phi.valid()[:, :, 0, 0].ravel(order="F")
    b = S["b"].ravel(order="F")
    res = np.abs(b - S["A"] @ xm).max() / np.abs(b).max()
    if S["singular"]:
        xm = xm - xm.mean()
    err = np.abs(xm - S["xd"]).max() / np.abs(S["xd"]).max()
    print("cc %s %s: oracle %d cycles, residual in the assembled matrix %.3e |b|, error against the direct solution %.3e" % (n, bcname, st.cycles, res, err))
    assert abs(S["lam"]) <= 1e-10 * np.abs(b).max()
    assert res <= 2e-11 and err <= 1e-8, (res, err)


def nd_fabs(n, S):
    lo, hi = box(n)
    pm = vo.ivec(list(S["per"]) + [0])
    sig, u = vo.Fab(lo, hi, 1, 1, dm=2), vo.Fab(lo, hi, 1, 2, dm=2)
    sig.valid()[:, :, 0, 0] = S["sig"]
    u.valid()[:, :, 0, :] = S["u"]
    vo.lib().vo_fill_boundary(sig.ref, pm)                  # periodic images only: zero beyond walls and outflow
    vo.lib().vo_fill_boundary(u.ref, pm)
    return pm, sig, u


@pytest.mark.parametrize("bcname", BCS)
@pytest.mark.parametrize("n", a2.SHAPES)
def test_nodal_operator_and_solution_2d(n, bcname):
    L = vo.lib()
    S = nd_system(n, bcname)
    NL, free = S["NL"], S["free"]
    lo, hi = box(n)
    pm, sig, u = nd_fabs(n, S)
    dx3 = vo.dvec(S["dx"] + [1.0])
    prm = default_params()
    nodal = (1, 1, 0)
    # K x: one residual of the oracle's solver with b = K_assembled x (module docstring)
    x = np.random.default_rng(2).standard_normal(NL.N); x[~free] = 0.0
    Kx = S["K"] @ x; Kx[~free] = 0.0
    rh, phi = vo.Fab(lo, hi, 1, 1, nodal, dm=2), vo.Fab(lo, hi, 1, 1, nodal, dm=2)
    rh.valid()[:, :, 0, 0] = -NL.to_grid(Kx)
    phi.valid()[:, :, 0, 0] = NL.to_grid(x)
    st = vo.CMgStat()
    L.vo_nd_solve(rh.ref, phi.ref, sig.ref, None, dx3, ell3(S["ell2"]), pm, C.c_double(0.0), C.c_double(-1.0), 0, 0, 0, prm.hg_nub, C.c_double(prm.hg_omega), 0, None, C.byref(st))
    assert st.cycles == 0 and st.res0 == np.abs(Kx).max()
    assert np.array_equal(phi.valid()[:, :, 0, 0], NL.to_grid(x)), "no sweep ran: phi comes back as it went in"
    assert st.res <= 1e-12 * np.abs(Kx).max(), "oracle K x differs from the element-assembled stiffness by %.3e (scale %.3e)" % (st.res, np.abs(Kx).max())
    # K phi = -D u against the direct solution
    rh.a[...] = 0.0; phi.a[...] = 0.0
    rc = L.vo_nd_solve(rh.ref, phi.ref, sig.ref, u.ref, dx3, ell3(S["ell2"]), pm, C.c_double(1e-12), C.c_double(-1.0), 100, prm.hg_nu1, prm.hg_nu2, prm.hg_nub,
                       C.c_double(prm.hg_omega), 1, None, C.byref(st))
    assert rc == 0, "nodal solve did not converge (%d cycles)" % st.cycles
    ym = NL.from_grid(phi.valid()[:, :, 0, 0])[free]
    if S["singular"]:
        ym = ym - ym.mean()
    err = np.abs(ym - S["yd"]).max() / np.abs(S["yd"]).max()
    print("nd %s %s: oracle %d cycles, error against the direct solution %.3e" % (n, bcname, st.cycles, err))
    assert abs(S["lam"]) <= 1e-9 * np.abs(S["w"][free]).max()
    assert err <= 1e-8, err


def test_the_element_weights_are_those_of_the_nine_point_operator():
    """per unit sigma and element: 2(fx + fy) on the node itself, -2fx + fy / fx - 2fy towards the x / y neighbour, -(fx + fy) across, f = 1/(6 h^2)"""
    h = (0.3, 0.5)
    Ke, G = a2.q1_element_matrices2(h)
    fx, fy = 1.0 / (6.0 * h[0] ** 2), 1.0 / (6.0 * h[1] ** 2)
    W = Ke / (h[0] * h[1])
    want = {0: 2.0 * (fx + fy), 1: -2.0 * fx + fy, 2: fx - 2.0 * fy, 3: -(fx + fy)}
    for a in range(4):
        for b in range(4):
            assert abs(W[a, b] - want[a ^ b]) <= 1e-14 * want[0], (a, b)
    assert np.abs(G.sum(axis=0)).max() == 0.0
