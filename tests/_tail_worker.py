"""child process of tests/test_tail_cycles_gpu.py: one cell-centred and one nodal solve per case under the launch-form switches of this process's environment
(they are read once per process).  One line per case: its name, the SHA-256 of phi without its ghost layer, the cycle count, the body the last tail cycle took
(vdn_last_tail_form of the testing build: 0 on global memory, 1 levels in LDS) and, with `oracle` as the first argument, the comparison against the oracle's
solve (tolerance and cycle rule of tests/test_projection_gpu.py::test_cc_solve / test_nd_solve).  `oracle-only`: the oracle's solves alone, no GPU (the check
that every case converges, run on the CPU before the cases were committed)."""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from oracle import voracle as vo
from tests._nd_prolong_worker import bubble_rho
from tests.util import Case, params_for

W, OUT, INL = 15, 12, 11
SHAPES = {"16": (16, 16, 16), "16x8x32": (16, 8, 32), "24": (24, 24, 24)}
BCS = {"walls": [[W, W], [W, W], [W, W]], "outz": [[W, W], [W, W], [W, OUT]], "inlet": [[INL, OUT], [W, W], [W, W]], "pery": [[W, W], [-1, -1], [W, W]]}
# name -> (solver, shape, boundary set, what is special).  aniso: dx in ratio 1 : 1.2 : 1 (the stencil's face weights are not zero); alpha: the viscous
# solves' cell coefficient; cg: the Krylov bottom solver, whose tail keeps the body on global memory
CASES = {}
for _s in SHAPES:
    for _b in BCS:
        CASES["cc-%s-%s" % (_s, _b)] = ("cc", _s, _b, "")
        CASES["nd-%s-%s" % (_s, _b)] = ("nd", _s, _b, "")
CASES["cc-16-walls-alpha"] = ("cc", "16", "walls", "alpha")
CASES["cc-16-walls-cg"] = ("cc", "16", "walls", "cg")
CASES["nd-16-outz-aniso"] = ("nd", "16", "outz", "aniso")
CASES["nd-16-walls-cg"] = ("nd", "16", "walls", "cg")


class OracleCase(Case):
    """the oracle's half of a Case: no library, no device"""

    def __init__(self, n, phys, seed, prm):
        self.n, self.phys, self.prm = tuple(n), phys, prm
        self.rng = np.random.default_rng(seed)
        self.lo, self.hi = (0, 0, 0), tuple(x - 1 for x in self.n)
        self.pmask = [1 if phys[d][0] == -1 else 0 for d in range(3)]
        self.obc = vo.make_bc(phys, 3, prm.nscal)
        self.opm = vo.ivec(self.pmask)
        self.dx = [1.0 / max(self.n)] * 3
        self.odx = vo.dvec(self.dx)

    def close(self):
        pass


def make_case(shape, bcname, special, with_gpu=True):
    kw = {}
    if special == "cg":
        kw = dict(mg_bottom_solver=2, hg_bottom_solver=2)
    prm = params_for(BCS[bcname], **kw)
    case = Case(SHAPES[shape], BCS[bcname], seed=29, iso=True, prm=prm) if with_gpu else OracleCase(SHAPES[shape], BCS[bcname], 29, prm)
    if special == "aniso":
        h = case.dx[0]
        case.dx = [h, 1.2 * h, h]
        case.odx = vo.dvec(case.dx)
    return case


def verdict_of(rc, cyc, st, r0, g, o):
    scale = np.abs(o - o.mean()).max()
    err = float(np.abs(g - o).max())
    ok = rc == 0 and cyc == st.cycles and r0 == st.res0 and err <= 1e-11 * scale
    return "%s:rc=%d,cycles=%d/%d,res0=%r/%r,err=%.3e,scale=%.3e" % ("ok" if ok else "FAIL", rc, cyc, st.cycles, r0, st.res0, err, scale)


def run_cc(case, special, mode):
    L = vo.lib()
    P = case.prm
    _, s = case.random_state()
    s.a[..., 0] = np.abs(s.a[..., 0]) + 0.5
    beta = [case.ofab(0, 1, tuple(1 if t == d else 0 for t in range(3))) for d in range(3)]
    L.vo_mk_mac_coeffs(s.ref, vo.fab_ptr_array(beta))
    rh = case.ofab(0, 1)
    rh.a[...] = case.rng.standard_normal(rh.a.shape)
    ell = vo.ellbc_of(case.obc)
    alpha = None
    if special == "alpha":
        alpha = case.ofab(0, 1)
        alpha.a[...] = 40.0 * (1.5 + 0.4 * np.sin(case.rng.uniform(0.0, 6.0, alpha.a.shape)))
    elif all(ell[d][sd] != 1 for d in range(3) for sd in range(2)):      # no Dirichlet face: make it solvable
        rh.a[...] -= rh.a.mean()
    cyc = r0 = 0
    g = None
    if mode != "oracle-only":
        from varden_amd import advance as adv
        gphi = case.gmf(case.ofab(1, 1))
        bc = [[ell[d][sd] for sd in range(2)] for d in range(3)]
        cyc, r0, r = adv.cc_solve(case.gmf(rh), gphi, [case.gmf(b) for b in beta], case.dx, bc, 1e-10, alpha=case.gmf(alpha) if alpha is not None else None)
        g = np.ascontiguousarray(gphi.to_numpy()[1:-1, 1:-1, 1:-1, 0])
    verdict = "-"
    if mode != "plain":
        ophi = case.ofab(1, 1)
        st = vo.CMgStat()
        L.vo_cc_solve_ab.restype = C.c_int
        rc = L.vo_cc_solve_ab(rh.ref, ophi.ref, alpha.ref if alpha is not None else None, vo.fab_ptr_array(beta), case.odx, ell, C.c_double(1e-10), C.c_double(-1.0),
                              P.mg_max_iter, P.mg_nu1, P.mg_nu2, P.mg_nub, P.mac_fmg, C.byref(st))
        o = ophi.a[1:-1, 1:-1, 1:-1, 0]
        verdict = ("ok:" if rc == 0 else "FAIL:") + "rc=%d,cycles=%d" % (rc, st.cycles) if g is None else verdict_of(rc, cyc, st, r0, g, o)
    return g, cyc, verdict


def run_nd(case, special, mode):
    L = vo.lib()
    P = case.prm
    u, _ = case.random_state()
    rhohalf = case.ofab(1, 1)
    rhohalf.a[..., 0] = bubble_rho(case)
    gpz = case.ofab(1, 3)
    L.vo_create_uvec(u.ref, u.ref, rhohalf.ref, gpz.ref, C.c_double(1.0), C.byref(case.obc), 1)
    L.vo_fill_boundary(u.ref, case.opm)
    coeffs = case.ofab(1, 1)
    coeffs.a[1:-1, 1:-1, 1:-1, 0] = 1.0 / rhohalf.a[1:-1, 1:-1, 1:-1, 0]
    L.vo_fill_boundary(coeffs.ref, case.opm)
    ell = vo.ellbc_of(case.obc)
    nodal = (1, 1, 1)
    cyc = r0 = 0
    g = None
    if mode != "oracle-only":
        from varden_amd import advance as adv
        grh, gphi = case.gmf(case.ofab(1, 1, nodal)), case.gmf(case.ofab(1, 1, nodal))
        bc = [[ell[d][sd] for sd in range(2)] for d in range(3)]
        cyc, r0, r = adv.nd_solve(grh, gphi, case.gmf(coeffs), case.gmf(u), case.dx, bc, 1e-11)
        g = np.ascontiguousarray(gphi.to_numpy()[1:-1, 1:-1, 1:-1, 0])
    verdict = "-"
    if mode != "plain":
        orh, ophi = case.ofab(1, 1, nodal), case.ofab(1, 1, nodal)
        st = vo.CMgStat()
        rc = L.vo_nd_solve(orh.ref, ophi.ref, coeffs.ref, u.ref, case.odx, ell, case.opm, C.c_double(1e-11), C.c_double(-1.0), P.hg_max_iter,
                           P.hg_nu1, P.hg_nu2, P.hg_nub, C.c_double(P.hg_omega), P.hg_fmg, (C.c_double * 2)(P.hg_omega_pre1, P.hg_omega_pre2), C.byref(st))
        o = ophi.a[1:-1, 1:-1, 1:-1, 0]
        verdict = ("ok:" if rc == 0 else "FAIL:") + "rc=%d,cycles=%d" % (rc, st.cycles) if g is None else verdict_of(rc, cyc, st, r0, g, o)
    return g, cyc, verdict


def run(name, mode):
    solver, shape, bcname, special = CASES[name]
    case = make_case(shape, bcname, special, mode != "oracle-only")
    g, cyc, verdict = (run_cc if solver == "cc" else run_nd)(case, special, mode)
    h, form = "-", -1
    if g is not None:
        h = hashlib.sha256(g.tobytes()).hexdigest()
        from varden_amd import capi
        f = capi.load().vdn_last_tail_form
        f.restype, f.argtypes = C.c_int, [C.c_int]
        form = f(0 if solver == "cc" else 1)
    print("CASE %s %s %d %d %s" % (name, h, cyc, form, verdict), flush=True)
    case.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "plain"
    for name in CASES:
        run(name, mode)
