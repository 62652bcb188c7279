"""Plane-averaged profiles (vdn_profiles): the grids with random fields the tests run it on (tests/_diagnostics_worker.py: Hier, with power-of-two spacings), the numpy
reference over the composite grid, and one or several ranks (threads, tests/_rank_threads.py) of the rank-independence test on ONE GPU
(tests/test_profiles_gpu.py::test_ranks_give_identical_bits).
argv: rank[,rank...] nranks idfile outprefix case"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests._diagnostics_worker import Hier, from_key, okey  # noqa: E402
from tests.children import rendezvous, save_rank  # noqa: E402

WALLS = [[15, 15]] * 3
EPS = 2.0 ** -53
SUM_GROUPS = ("volume", "s", "ss", "u", "ru", "ruu", "sua")
KEY_GROUPS = ("s_min", "s_max", "u_min", "u_max")

# one level, dm = 3: a box none of whose extents is a multiple of the wave width and whose planes are smaller than a workgroup; 32 x 16 x 24 cut into 2 x 1 x 3 boxes
ONE_LEVEL = {"one-box": ((12, 20, 8), [((0, 0, 0), (11, 19, 7))]),
             "six-boxes": ((32, 16, 24), [((16 * i, 0, 8 * k), (16 * i + 15, 15, 8 * k + 7)) for k in range(3) for i in range(2)])}
# three levels: a 16^3 base in two boxes split along x; two level-1 boxes that are not aligned with each other and abut nowhere; one level-2 box strictly inside the
# first.  Along every axis some bins are reached by one level, some by two, some by three, and every r from 1 to 4 occurs
AMR3 = (16, [[((0, 0, 0), (7, 15, 15)), ((8, 0, 0), (15, 15, 15))],
             [((8, 8, 4), (19, 23, 15)), ((20, 8, 16), (27, 15, 31))],
             [((20, 20, 12), (35, 43, 27))]])
# dm = 2, one level: 24 x 40 in two boxes
FLAT = ((24, 40), [((0, 0, 0), (23, 19, 0)), ((0, 20, 0), (23, 39, 0))])
WIDE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


def hier(pkg, nbase, boxes, **kw):
    """Hier with every ghost cell NaN and spacings that are powers of two (2^-3, 2^-2, 2^-4 on level 0, halved per level): a cell's weight and a bin's volume are exact"""
    H = Hier(pkg, nbase, boxes, nan_ghosts=True, **kw)
    H.dx = [[2.0 ** -((3, 2, 4)[d] + l) for d in range(H.dm)] for l in range(H.nlev)]
    return H


def profiles(H, axis):
    return H.pkg.advance.profiles(H.mla, H.u, H.s, H.dx, axis)


def row_terms(H, U, S, l, axis):
    """level l: {group: [array over the level's domain per row]} of the terms vdn_profiles sums (products left to right, then the weight), the values the extrema run
    over, and the weight w_l"""
    dm, ns, L = H.dm, H.nscal, H.nlev - 1
    w = float(np.prod(H.dx[l])) / (1 << (L - l))
    u, s = [U[l][..., d] for d in range(dm)], [S[l][..., c] for c in range(ns)]
    T = dict(volume=[np.full(U[l].shape[:3], w)], s=[s[c] * w for c in range(ns)], ss=[(s[c] * s[c]) * w for c in range(ns)], u=[u[d] * w for d in range(dm)],
             ru=[(s[0] * u[d]) * w for d in range(dm)], ruu=[((s[0] * u[d]) * u[e]) * w for d in range(dm) for e in range(d, dm)],
             sua=[(s[c] * u[axis]) * w for c in range(1, ns)], s_min=s, s_max=s, u_min=u, u_max=u)
    return T, w


def _plane_sum(a, axis):
    """the sum over the two directions other than `axis`, in extended precision: numpy.longdouble where it is wider than double, math.fsum otherwise"""
    other = tuple(d for d in range(3) if d != axis)
    if WIDE:
        return a.astype(np.longdouble).sum(axis=other)
    b = np.moveaxis(a, axis, 0).reshape(a.shape[axis], -1)
    return np.array([math.fsum(r) for r in b])


def reference(H, axis):
    """numpy over to_numpy() of the same multifabs and the composite mask from the box lists: per group an array (rows, nbins) -- sums in extended precision (rounded to
    double at the end), extrema as exact values --, cells (nbins,), abs_sum (the sum of |term| per sum row and bin) and nterms (the number of terms per bin = cells)"""
    U, S, M = H.gather(H.u), H.gather(H.s), H.composite()
    L = H.nlev - 1
    nbins = H.n[0][axis] << L
    other = tuple(d for d in range(3) if d != axis)
    ref = {g: None for g in SUM_GROUPS + KEY_GROUPS}
    cells = np.zeros(nbins, dtype=np.int64)
    acc, absum, keys = {}, {}, {}
    for l in range(H.nlev):
        T, _ = row_terms(H, U, S, l, axis)
        r = 1 << (L - l)
        cells += np.repeat(M[l].sum(axis=other), r)
        for g in SUM_GROUPS:
            for i, t in enumerate(T[g]):
                t = np.where(M[l], t, 0.0)                           # a covered cell (or one outside the level's boxes: NaN in gather) contributes nothing
                acc[g, i] = acc.get((g, i), 0) + np.repeat(_plane_sum(t, axis), r)
                absum[g, i] = absum.get((g, i), 0) + np.repeat(_plane_sum(np.abs(t), axis), r)
        for g in KEY_GROUPS:
            for i, v in enumerate(T[g]):
                k = okey(np.where(M[l], v, 0.0)).reshape(v.shape)
                if g.endswith("min"):
                    k = np.repeat(np.where(M[l], k, np.uint64(2 ** 64 - 1)).min(axis=other), r)
                    keys[g, i] = k if (g, i) not in keys else np.minimum(keys[g, i], k)
                else:
                    k = np.repeat(np.where(M[l], k, np.uint64(0)).max(axis=other), r)
                    keys[g, i] = k if (g, i) not in keys else np.maximum(keys[g, i], k)
    nrows = {g: len([k for k in list(acc) + list(keys) if k[0] == g]) for g in SUM_GROUPS + KEY_GROUPS}
    for g in SUM_GROUPS:
        ref[g] = np.array([np.asarray(acc[g, i], dtype=np.float64) for i in range(nrows[g])]).reshape(nrows[g], nbins)
    for g in KEY_GROUPS:
        ref[g] = np.array([[from_key(k) for k in keys[g, i]] for i in range(nrows[g])]).reshape(nrows[g], nbins)
    ab = {g: np.array([np.asarray(absum[g, i], dtype=np.float64) for i in range(nrows[g])]).reshape(nrows[g], nbins) for g in SUM_GROUPS}
    return ref, cells, ab


def group(P, g):
    """a row group of a Profiles object as (rows, nbins)"""
    a = P[g]
    return a.reshape(1, -1) if a.ndim == 1 else a


def check(P, H, axis, what=""):
    """every row of a Profiles object against the reference: cells and extrema as 64-bit patterns, sums within (n + 4) 2^-53 sum |term| per bin and row, n the number
    of terms in the bin -- n - 1 roundings of a recursive sum in any order or tree, at most three inside a term (two products and the weight), one for the reference's
    own conversion; fused multiply-adds would only reduce the count.  Derived, not measured"""
    ref, cells, ab = reference(H, axis)
    assert P.cells.dtype == np.int64 and np.array_equal(P.cells, cells), (what, axis, P.cells, cells)
    for g in KEY_GROUPS:
        got = group(P, g)
        assert got.shape == ref[g].shape, (what, g, got.shape, ref[g].shape)
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(ref[g]).view(np.uint64)), (what, axis, g, got, ref[g])
    worst = 0.0
    for g in SUM_GROUPS:
        got = group(P, g)
        assert got.shape == ref[g].shape, (what, g, got.shape, ref[g].shape)
        bound = (cells[None, :] + 4) * EPS * ab[g]
        diff = np.abs(got - ref[g])
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, diff / bound, 0.0))))
        bad = np.argwhere(~(diff <= bound))
        assert bad.size == 0, (what, axis, g, bad[:4], got[tuple(bad[0])], ref[g][tuple(bad[0])], bound[tuple(bad[0])])
    print("%s axis %d: %d bins, %d rows; the largest |device - numpy| / bound = %.3f" % (what, axis, len(cells), P.rows.shape[0], worst))
    return ref, cells, ab


def all_bits(P):
    """every figure of a Profiles object as its 64-bit pattern: the rows, then the counts"""
    return np.concatenate([np.ascontiguousarray(P.rows).view(np.uint64).ravel(), P.cells.astype(np.uint64)])


def main():
    ranks, nranks = [int(r) for r in sys.argv[1].split(",")], int(sys.argv[2])
    from tests._rank_threads import run_ranks
    run_ranks(ranks, lambda rank, pkg: one_rank(rank, nranks, pkg), os.path.dirname(sys.argv[4]))


def one_rank(rank, nranks, pkg):
    idfile, outprefix = sys.argv[3], sys.argv[4]
    prm = pkg.capi.default_params(nscal=3)
    comm_id = rendezvous(pkg.boxlib, prm, rank, nranks, idfile)
    H = hier(pkg, AMR3[0], AMR3[1], nscal=3, seed=7, rank=rank, nranks=nranks, comm_id=comm_id)
    out = {}
    for axis in range(3):
        out["axis%d" % axis] = all_bits(profiles(H, axis))
        out["again%d" % axis] = all_bits(profiles(H, axis))
    save_rank(outprefix, rank, out)
    H.close()
    if nranks > 1:
        pkg.boxlib.comm_finalize()


if __name__ == "__main__":
    main()
