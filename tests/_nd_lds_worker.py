"""child process of tests/test_nd_lds_levels_gpu.py: the nodal solve of every case under the launch-form switches of this process's environment (they are read
once per process); one line per case: its name, the SHA-256 of phi, the cycle count, the levels of that solve that ran as kk_nd_lds_down / kk_nd_lds_up
(vdn_nd_lds_levels of the testing build: bit l) and, with `oracle` as the first argument, the comparison against the oracle's nodal solve (tolerance and cycle
rule of tests/test_projection_gpu.py::test_nd_solve, as tests/_nd_prolong_worker.py does it)"""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from oracle import voracle as vo
from tests._nd_prolong_worker import BCS, bubble_rho
from tests.util import Case, params_for

# name -> (cells of the finest level, hg_fmg)
SHAPES = {"32": ((32, 32, 32), 1), "64": ((64, 64, 64), 1), "64-nofmg": ((64, 64, 64), 0), "128x32x32": ((128, 32, 32), 1), "48x32x80": ((48, 32, 80), 1),
          "40": ((40, 40, 40), 1)}


def run(shape, bcname, with_oracle):
    n, fmg = SHAPES[shape]
    case = Case(n, BCS[bcname], seed=23, iso=True, prm=params_for(BCS[bcname], hg_fmg=fmg))
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
    from varden_amd import advance as adv
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
    f = capi.load().vdn_nd_lds_levels
    f.restype, f.argtypes = C.c_uint, []
    print("CASE %s-%s %s %d %d %s" % (shape, bcname, h, cyc, f(), verdict), flush=True)
    case.close()


if __name__ == "__main__":
    with_oracle = len(sys.argv) > 1 and sys.argv[1] == "oracle"
    for shape in SHAPES:
        for bcname in BCS:
            run(shape, bcname, with_oracle)
