"""Extra tracers (nscal > 2): the smooth, distinct fields the tests give the tracers, and one or several ranks (threads, tests/_rank_threads.py) of a
multi-rank hierarchy run with nscal = 5 on ONE GPU (tests/test_tracers_gpu.py::test_tracers_on_several_ranks_reproduce_one_rank).
argv: rank[,rank...] nranks idfile outprefix fixed|tagged"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.children import rendezvous, save_rank  # noqa: E402


def tracer_value(m, X, Y, Z):
    """field of tracer number m >= 1 at the physical points (X, Y, Z): a smooth product of modes that differs from tracer to tracer, between 0.1 and 0.9"""
    a, b, c = 1 + m % 3, 1 + (2 * m) % 3, 1 + (m + 1) % 2
    return (0.5 + 0.25 * np.sin(2.0 * np.pi * a * X + 0.7 * m) * np.cos(2.0 * np.pi * b * Y + 0.3 * m)
            + 0.15 * np.cos(2.0 * np.pi * c * Z + 1.1 * m) * np.sin(np.pi * X + 0.2 * m))


def cell_centres(lo, shape, dx, ng=3):
    """physical cell centres of an array of `shape` (ghost cells included) whose first valid cell is lo"""
    ax = [dx[d] * (lo[d] - ng + np.arange(shape[d]) + 0.5) for d in range(3)]
    return np.meshgrid(*ax, indexing="ij")


def set_tracers(s, lo, dx, fields, ng=3, zuniform=False):
    """s[..., j] = tracer_value(fields[j - 1]) for j = 1 .. nc - 1 (component 0, the density, is left alone); every cell of the array, ghosts included.
    zuniform: the tracers depend on x and y only (the z-uniform copies of 2-D problems)"""
    shape = s.shape[:3]
    if s.shape[2] == 1:                      # a dm = 2 array: one z-plane, no ghost cells along z
        X, Y, _ = cell_centres((lo[0], lo[1], 0), (shape[0], shape[1], 1), (dx[0], dx[1], 1.0), ng)
        Z = np.zeros_like(X)
    else:
        X, Y, Z = cell_centres(lo, shape, dx, ng)
        if zuniform:
            Z = np.zeros_like(Z)
    for j in range(1, s.shape[3]):
        s[..., j] = tracer_value(fields[j - 1], X, Y, Z)
    return s


def init_with_tracers(fields, prob_type=1, base=None, initdata=None):
    """init_fn(level, box_lo, box_shape, dx) of driver.VardenAMR / voracle.SimML: initdata (prob_type) for u and the density, tracer_value(fields[j - 1]) for
    scalar component j >= 1.  base: an init_fn to start from (e.g. driver.extruded_initdata; the tracers then depend on x and y only); initdata: the
    driver's initdata_numpy (a rank's private copy of the package)"""
    if initdata is None:
        from varden_amd.driver import initdata_numpy as initdata
    ns = len(fields) + 1

    def fn(level, lo, nb, dx):
        if base is None:
            u, s = initdata(nb, dx, prob_type, 3, ns, lo=lo)
        else:
            u, s = base(level, lo, nb, dx)
        return u, set_tracers(np.array(s, order="F"), lo, dx, fields, zuniform=base is not None)
    return fn


FIVE = (1, 2, 3, 4, 5)                       # nscal = 5: the density and four tracers, each with its own field


def main():
    ranks, nranks = [int(r) for r in sys.argv[1].split(",")], int(sys.argv[2])
    from tests._rank_threads import run_ranks
    run_ranks(ranks, lambda rank, pkg: one_rank(rank, nranks, pkg), os.path.dirname(sys.argv[4]))


def one_rank(rank, nranks, pkg):
    idfile, outprefix, mode = sys.argv[3], sys.argv[4], sys.argv[5]
    bl, driver = pkg.boxlib, pkg.driver
    prm = pkg.capi.default_params(cflfac=0.9, visc_coef=0.001, diff_coef=0.001, nscal=5)
    comm_id = rendezvous(bl, prm, rank, nranks, idfile)
    walls = [[bl.NO_SLIP_WALL] * 2] * 3
    init = init_with_tracers(FIVE[:4], initdata=driver.initdata_numpy)
    if mode == "tagged":     # grids from the tagged bubble on a 32^3 base in four boxes, regridding every second step
        base = [((0, 0, 0), (15, 15, 31)), ((16, 0, 0), (31, 15, 31)), ((0, 16, 0), (15, 31, 31)), ((16, 16, 0), (31, 31, 31))]
        levels = driver.VardenAMR.tagged_grids(32, walls, prm, max_levs=2, buf_wid=2, max_grid_size=16, rank=rank, nranks=nranks, comm_id=comm_id, base_boxes=base)
        G = driver.VardenAMR(32, levels[0], walls, params=prm, finer_levels=levels[1:], base_boxes=base, init_iter=1, do_initial_projection=1,
                             regrid_int=2, max_levs=2, max_grid_size=16, rank=rank, nranks=nranks, comm_id=comm_id, init_fn=init)
        nsteps = 3
    else:                    # a fixed two-level hierarchy, level 0 in four boxes
        base = [((0, 0, 0), (7, 7, 15)), ((8, 0, 0), (15, 7, 15)), ((0, 8, 0), (7, 15, 15)), ((8, 8, 0), (15, 15, 15))]
        fine = [((8, 8, 8), (15, 23, 23)), ((16, 8, 8), (23, 15, 23)), ((16, 16, 8), (23, 23, 23))]
        G = driver.VardenAMR(16, fine, walls, params=prm, base_boxes=base, init_iter=1, do_initial_projection=1,
                             rank=rank, nranks=nranks, comm_id=comm_id, init_fn=init)
        nsteps = 2
    dts = []
    for _ in range(nsteps):
        G.step()
        dts.append(G.dt)
    out = {"dt": np.array(dts), "nboxes": np.array([len(b) for b in G.boxes]), "nregrids": np.array([G.nregrids])}
    for n in range(G.nlev):
        for li, gi in enumerate(G.local[n]):
            out["u%d_%d" % (n, gi)] = G.unew[n].to_numpy(li)[3:-3, 3:-3, 3:-3]
            out["s%d_%d" % (n, gi)] = G.snew[n].to_numpy(li)[3:-3, 3:-3, 3:-3]
            out["p%d_%d" % (n, gi)] = G.p[n].to_numpy(li)[1:-1, 1:-1, 1:-1]
    save_rank(outprefix, rank, out)
    G.close()


if __name__ == "__main__":
    main()
