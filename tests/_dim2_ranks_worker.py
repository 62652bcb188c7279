"""one or several ranks of a dm = 2 run on ONE GPU (tests/test_dim2_boxlists_gpu.py), after tests/_multirank_worker.py: the ranks are processes,
the transport is the RCCL test double tests/fake_rccl (VDN_RCCL_LIB), the rendezvous a file.
argv: rank nranks idfile outprefix bx by n nsteps bcname"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.children import rendezvous, save_rank  # noqa: E402

BCS = {"walls": [[15, 15], [15, 15]], "periodic": [[-1, -1], [15, 15]]}


def main():
    rank, nranks, idfile, outprefix = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    decomp = (int(sys.argv[5]), int(sys.argv[6]), 1)
    n, nsteps, bc = int(sys.argv[7]), int(sys.argv[8]), BCS[sys.argv[9]]
    from varden_amd import boxlib as bl, driver
    from varden_amd.capi import default_params
    prm = default_params(dm=2, cflfac=0.9, visc_coef=0.001)
    comm_id = rendezvous(bl, prm, rank, nranks, idfile)
    G = driver.Varden(n, [bc[0], bc[1], [0, 0]], prm, prob_type=1, init_shrink=0.1, init_iter=1, decomp=decomp, rank=rank, nranks=nranks, comm_id=comm_id)
    dts = []
    for _ in range(nsteps):
        G.step()
        dts.append(G.dt)
    out = {"dt": np.array(dts)}
    for li, gi in enumerate(G.local):
        out["u%d" % gi] = G.uold[0].to_numpy(li)[3:-3, 3:-3]
        out["s%d" % gi] = G.sold[0].to_numpy(li)[3:-3, 3:-3]
        out["gp%d" % gi] = G.gp[0].to_numpy(li)[1:-1, 1:-1]
        out["p%d" % gi] = G.p[0].to_numpy(li)[1:-1, 1:-1]
    save_rank(outprefix, rank, out)
    G.close()


if __name__ == "__main__":
    main()
