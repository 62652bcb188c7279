"""child process of tests/test_nd_prolong_fused_gpu.py: the nodal solve of every case under the launch-form switches of this process's environment
(they are read once per process); one line per case: its name, the SHA-256 of phi, the cycle count, the levels of that solve that took the prolonging march
(vdn_nd_prolong_fused_levels of the testing build: bit l) and, with `oracle` as the first argument, the comparison against the oracle's nodal solve (tolerance and cycle rule of tests/test_projection_gpu.py::test_nd_solve)"""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from oracle import voracle as vo
from tests.util import Case
from varden_amd import advance as adv

W, OUT = 15, 12
SHAPES = {"128x16x24": (128, 16, 24), "260x8x12": (260, 8, 12), "128x16x28": (128, 16, 28)}
BCS = {"walls": [[W, W], [W, W], [W, W]], "outx": [[W, OUT], [W, W], [W, W]], "outy": [[W, W], [OUT, W], [W, W]], "outz": [[W, W], [W, W], [W, OUT]]}


def bubble_rho(case):
    """the density of the bubble problem: 2 inside a sphere, 1 outside, a tanh profile between (cell centres, one ghost cell)"""
    n, dx = case.n, case.dx
    ax = [(np.arange(-1, n[d] + 1) + 0.5) * dx[d] for d in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    cen = [0.5 * n[d] * dx[d] for d in range(3)]
    r = np.sqrt((X - cen[0]) ** 2 + (Y - 0.8 * cen[1]) ** 2 + (Z - 1.1 * cen[2]) ** 2)
    rad = 0.6 * min(cen)
    return 1.0 + 0.5 * (1.0 + np.tanh((rad - r) / (2.0 * dx[0])))


def run(shape, bcname, with_oracle):
    case = Case(SHAPES[shape], BCS[bcname], seed=21, iso=True)
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
    grh, gphi = case.gmf(case.ofab(1, 1, nodal)), case.gmf(case.ofab(1, 1, nodal))
    bc = [[ell[d][sd] for sd in range(2)] for d in range(3)]
    cyc, r0, r = adv.nd_solve(grh, gphi, case.gmf(coeffs), case.gmf(u), case.dx, bc, 1e-11)
    g = gphi.to_numpy()
    h = hashlib.sha256(np.ascontiguousarray(g).tobytes()).hexdigest()
    verdict = "-"
    if with_oracle:
        orh, ophi = case.ofab(1, 1, nodal), case.ofab(1, 1, nodal)
        st = vo.CMgStat()
        rc = L.vo_nd_solve(orh.ref, ophi.ref, coeffs.ref, u.ref, case.odx, ell, case.opm, C.c_double(1e-11), C.c_double(-1.0), 100,
                           P.hg_nu1, P.hg_nu2, P.hg_nub, C.c_double(P.hg_omega), P.hg_fmg, (C.c_double * 2)(P.hg_omega_pre1, P.hg_omega_pre2), C.byref(st))
        gv, o = g[1:-1, 1:-1, 1:-1, 0], ophi.a[1:-1, 1:-1, 1:-1, 0]
        scale = np.abs(o - o.mean()).max()
        err = float(np.abs(gv - o).max())
        ok = rc == 0 and cyc == st.cycles and r0 == st.res0 and err <= 1e-11 * scale
        verdict = "%s:rc=%d,cycles=%d/%d,res0=%r/%r,err=%.3e,scale=%.3e" % ("ok" if ok else "FAIL", rc, cyc, st.cycles, r0, st.res0, err, scale)
    from varden_amd import capi
    f = capi.load().vdn_nd_prolong_fused_levels
    f.restype, f.argtypes = C.c_uint, []
    print("CASE %s-%s %s %d %d %s" % (shape, bcname, h, cyc, f(), verdict), flush=True)
    case.close()


if __name__ == "__main__":
    with_oracle = len(sys.argv) > 1 and sys.argv[1] == "oracle"
    for shape in SHAPES:
        for bcname in BCS:
            run(shape, bcname, with_oracle)
