"""one or several ranks (threads, tests/_rank_threads.py) of make_new_grids_by on ONE GPU (tests/test_tag_criteria_gpu.py::test_two_ranks_return_the_boxes_of_one):
a 32^3 level in eight 16^3 boxes dealt to the ranks, a smooth velocity with a vorticity ridge, one vorticity criterion.  argv: rank[,rank...] nranks idfile outprefix"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.children import rendezvous, save_rank  # noqa: E402


def main():
    ranks, nranks = [int(r) for r in sys.argv[1].split(",")], int(sys.argv[2])
    from tests._rank_threads import run_ranks
    run_ranks(ranks, lambda rank, pkg: one_rank(rank, nranks, pkg), os.path.dirname(sys.argv[4]))


def velocity(lo, n, h):
    """a shear layer bent in z: valid cells and three ghost layers of the box at `lo`, from the cell centres (so every rank and every box agree)"""
    ax = [h * (lo[d] - 3 + np.arange(n[d] + 6) + 0.5) for d in range(3)]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    u = np.zeros(X.shape + (3,), order="F")
    u[..., 0] = np.tanh((Y - 0.5 - 0.1 * np.sin(2.0 * np.pi * Z)) / 0.08)
    u[..., 1] = 0.1 * np.sin(2.0 * np.pi * X)
    u[..., 2] = 0.05 * np.cos(2.0 * np.pi * (X + Y))
    return u


def one_rank(rank, nranks, pkg):
    idfile, outprefix = sys.argv[3], sys.argv[4]
    bl, adv, driver = pkg.boxlib, pkg.advance, pkg.driver
    prm = pkg.capi.default_params()
    comm_id = rendezvous(bl, prm, rank, nranks, idfile)
    bl.initialize(prm, rank, nranks, 0)
    if nranks > 1:
        bl.comm_init(comm_id)
    n, h = 32, 1.0 / 32
    boxes = [((i, j, k), (i + 15, j + 15, k + 15)) for k in (0, 16) for j in (0, 16) for i in (0, 16)]
    owner = driver.distribute(boxes, nranks)
    phys = [[bl.PERIODIC] * 2, [bl.NO_SLIP_WALL] * 2, [bl.PERIODIC] * 2]
    mla = bl.MLLayout([((0, 0, 0), (n - 1,) * 3)], [boxes], owner=[owner], pmask=(1, 0, 1))
    bct = bl.BCTower(mla, phys)
    u, s = bl.MultiFab(mla, 0, 3, 3), bl.MultiFab(mla, 0, 2, 3)
    s.setval(1.0, all=True)
    for li, gi in enumerate([i for i, o in enumerate(owner) if o == rank]):
        u.from_numpy(velocity(boxes[gi][0], (16, 16, 16), h), li)
    new, nt = adv.make_new_grids_by(s, u, [h] * 3, bct, 1, [dict(field="vorticity", gt=6.0)], buf_wid=2, nest=0, max_grid_size=16)
    tags = adv.tag_boxes_by(s, u, [h] * 3, bct, 1, [dict(field="vorticity", gt=6.0)])
    save_rank(outprefix, rank, {"boxes": np.array(new, dtype=np.int64).reshape(-1, 6), "ntagged": np.array([nt]), "tags": tags,
                                "nlocal": np.array([u.nfabs()])})
    for m in (u, s):
        m.destroy()
    bct.destroy()
    mla.destroy()
    if nranks > 1:
        bl.comm_finalize()


if __name__ == "__main__":
    main()
