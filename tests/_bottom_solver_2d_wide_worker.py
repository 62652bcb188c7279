"""one rank of tests/test_bottom_solver_2d_wide_gpu.py::test_two_ranks_reproduce_one_rank_bits_with_grid_wide_cg_bottoms: the dm = 2 bubble on (284, 150) cells in
two boxes of 142 x 150 with mg_bottom_solver = hg_bottom_solver = 2 (every rank holds the gathered level; its bottom of 142 x 75 cells / 143 x 76 nodes is solved over
the whole GPU), two steps; ranks are processes on ONE GPU, the transport is the RCCL test double tests/fake_rccl (VDN_RCCL_LIB), the rendezvous a file.
argv: rank nranks idfile outprefix"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.children import rendezvous, save_rank  # noqa: E402


def main():
    rank, nranks, idfile, outprefix = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    from varden_amd import advance as adv
    from varden_amd import boxlib as bl
    from varden_amd import driver
    from varden_amd.capi import default_params
    prm = default_params(dm=2, cflfac=0.9, visc_coef=0.001, mg_bottom_solver=2, hg_bottom_solver=2)
    comm_id = rendezvous(bl, prm, rank, nranks, idfile)
    n = (284, 150)
    h = 1.0 / max(n)
    G = driver.Varden(n, [[15, 15], [15, 15], [0, 0]], prm, prob_type=1, prob_hi=(n[0] * h, n[1] * h, 1.0), init_shrink=0.1, init_iter=1,
                      decomp=(2, 1, 1), rank=rank, nranks=nranks, comm_id=comm_id)
    dts, mac, hg, forms = [], [], [], []
    for _ in range(2):
        G.step()
        dts.append(G.dt)
        mac.append(adv.last_bottom_stats("mac")["iters"]); hg.append(adv.last_bottom_stats("hg")["iters"])
        forms += [adv.last_bottom_form("mac"), adv.last_bottom_form("hg")]
    out = {"dt": np.array(dts), "mac_iters": np.array(mac), "hg_iters": np.array(hg), "forms": np.array(forms)}
    for li, gi in enumerate(G.local):
        out["u%d" % gi] = G.unew[0].to_numpy(li)[3:-3, 3:-3]
        out["s%d" % gi] = G.snew[0].to_numpy(li)[3:-3, 3:-3]
        out["gp%d" % gi] = G.gp[0].to_numpy(li)[1:-1, 1:-1]
        out["p%d" % gi] = G.p[0].to_numpy(li)[1:-1, 1:-1]
    save_rank(outprefix, rank, out)
    G.close()


if __name__ == "__main__":
    main()
