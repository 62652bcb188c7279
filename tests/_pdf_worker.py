"""PDFs and conditional sums by value (vdn_pdf, vdn_pdf2): the slot rule of csrc/pdf_bin.h restated in numpy, the numpy reference over the composite grid of the grids
of tests/_profiles_worker.py, and one or several ranks (threads, tests/_rank_threads.py) of the rank-independence test on ONE GPU
(tests/test_pdf_gpu.py::test_ranks_give_identical_bits).
argv: rank[,rank...] nranks idfile outprefix"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests._profiles_worker import AMR3, EPS, WIDE, hier  # noqa: E402
from tests.children import rendezvous, save_rank  # noqa: E402

SUM_GROUPS = ("q", "s", "u", "ru", "ke")
FIELDS = ("scalar", "velocity", "magvel", "vorticity")
# the axes the rank workers and the two-call test run: (field, comp, lo, hi, nbins)
RANK_AXES = (("scalar", 0, -0.75, 0.8, 64), ("velocity", 2, -0.5, 0.9, 7), ("magvel", 0, 0.2, 1.5, 256), ("vorticity", 0, 1.0, 400.0, 256))
RANK_PAIR = (("scalar", 0, -0.75, 0.8, 64), ("velocity", 2, -0.5, 0.9, 5))


def slots(q, lo, hi, nbins):
    """pdf_slot of csrc/pdf_bin.h in float64: -1 for NaN, 0 below lo, nbins + 1 at and above hi, else 1 + min(floor((q - lo) / w), nbins - 1) with w = (hi - lo) / nbins
    formed once -- a true division, the comparison with nbins - 1 made on the float"""
    q = np.asarray(q, dtype=np.float64)
    w = (float(hi) - float(lo)) / nbins
    with np.errstate(all="ignore"):
        m = np.minimum(np.floor((q - float(lo)) / w), float(nbins - 1))
    fin = ~np.isnan(q)
    out = np.full(q.shape, -1, dtype=np.int64)
    out[fin & (q < lo)] = 0
    out[fin & (q >= hi)] = nbins + 1
    inside = fin & (q >= lo) & (q < hi)
    out[inside] = 1 + m[inside].astype(np.int64)
    return out


def vorticity(H):
    """vdn_make_vorticity of every level into a multifab (it fills the same-level and physical ghost cells of u, which vdn_pdf then reads), gathered"""
    W = []
    for l in range(H.nlev):
        w = H.bl.MultiFab(H.mla, l, 1, 0)
        H.pkg.advance.make_vorticity(w, 0, H.u[l], H.dx[l], H.bct)
        W.append(w)
    out = H.gather(W)
    for w in W:
        w.destroy()
    return out


def bin_field(H, U, S, field, comp):
    """q per level over the level's domain: the expressions of include/varden_amd.h in float64 (numpy's sqrt is correctly rounded, as the device's is); the vorticity is
    vdn_make_vorticity's own output"""
    if field == "scalar":
        return [S[l][..., comp] for l in range(H.nlev)]
    if field == "velocity":
        return [U[l][..., comp] for l in range(H.nlev)]
    if field == "magvel":
        out = []
        for l in range(H.nlev):
            q2 = U[l][..., 0] * U[l][..., 0] + U[l][..., 1] * U[l][..., 1]
            if H.dm == 3:
                q2 = q2 + U[l][..., 2] * U[l][..., 2]
            out.append(np.sqrt(q2))
        return out
    return [w[..., 0] for w in vorticity(H)]


def row_terms(H, U, S, Q, l):
    """level l: {group: [array over the level's domain per row]} of the terms vdn_pdf sums: products as written, then the cell volume"""
    dm, ns = H.dm, H.nscal
    dv = float(np.prod(H.dx[l]))
    u, s = [U[l][..., d] for d in range(dm)], [S[l][..., c] for c in range(ns)]
    q2 = u[0] * u[0] + u[1] * u[1]
    if dm == 3:
        q2 = q2 + u[2] * u[2]
    return dict(q=[Q[l] * dv], s=[s[c] * dv for c in range(ns)], u=[u[d] * dv for d in range(dm)], ru=[(s[0] * u[d]) * dv for d in range(dm)],
                ke=[((0.5 * s[0]) * q2) * dv]), dv


def _slot_sums(t, sl, nslot):
    """the sum of t over the cells of every slot in extended precision: numpy.longdouble where it is wider than double, math.fsum otherwise"""
    order = np.argsort(sl, kind="stable")
    ss, ts = sl[order], t[order]
    start = np.searchsorted(ss, np.arange(nslot + 1))
    out = np.zeros(nslot, dtype=np.longdouble if WIDE else np.float64)
    for m in range(nslot):
        if start[m + 1] > start[m]:
            seg = ts[start[m]:start[m + 1]]
            with np.errstate(invalid="ignore"):
                out[m] = seg.astype(np.longdouble).sum() if WIDE else (math.fsum(seg) if np.isfinite(seg).all() else seg.sum())
    return out


def reference(H, field, comp, lo, hi, nbins):
    """numpy over to_numpy() of the same multifabs and the composite mask from the box lists: cells (nlev, nbins + 2), nan_cells, volume (nbins + 2,), per sum group an
    array (rows, nbins + 2) added in extended precision and rounded to double at the end, abs_sum (the sum of |term| per row and slot)"""
    with np.errstate(invalid="ignore"):
        U, S, M = H.gather(H.u), H.gather(H.s), H.composite()
        Q = bin_field(H, U, S, field, comp)
    nslot = nbins + 2
    cells, nan_cells = np.zeros((H.nlev, nslot), dtype=np.int64), 0
    acc, absum = {}, {}
    for l in range(H.nlev):
        with np.errstate(invalid="ignore", over="ignore"):
            T, dv = row_terms(H, U, S, Q, l)
        sl = slots(Q[l][M[l]], lo, hi, nbins)
        nan_cells += int((sl < 0).sum())
        keep = sl >= 0
        cells[l] = np.bincount(sl[keep], minlength=nslot)
        for g in SUM_GROUPS:
            for i, t in enumerate(T[g]):
                t = t[M[l]][keep]
                acc[g, i] = acc.get((g, i), 0) + _slot_sums(t, sl[keep], nslot)
                absum[g, i] = absum.get((g, i), 0) + _slot_sums(np.abs(t), sl[keep], nslot)
    volume = np.zeros(nslot)
    for l in range(H.nlev):                                       # ascending, in double, as the library forms it
        volume = volume + cells[l].astype(np.float64) * float(np.prod(H.dx[l]))
    nrows = {g: len([k for k in acc if k[0] == g]) for g in SUM_GROUPS}
    ref = {g: np.array([np.asarray(acc[g, i], dtype=np.float64) for i in range(nrows[g])]).reshape(nrows[g], nslot) for g in SUM_GROUPS}
    ab = {g: np.array([np.asarray(absum[g, i], dtype=np.float64) for i in range(nrows[g])]).reshape(nrows[g], nslot) for g in SUM_GROUPS}
    return ref, cells, nan_cells, volume, ab


def group(P, g):
    a = P[g]
    return a.reshape(1, -1) if a.ndim == 1 else a


def check(P, H, field, comp, lo, hi, nbins, what=""):
    """a Pdf object against the reference: cells per level, nan_cells and the volume row exactly; every sum row within (n + 8) 2^-53 sum |term| per slot and row, n the
    slot's cell count -- n - 1 roundings of a sum in any order or tree, at most 7 inside a term (ke in 3-D: three squares, two additions, the product with 0.5 rho
    (0.5 rho itself is exact), the volume), one for the reference's own conversion.  Derived, not measured.  Where the reference is not finite (a planted Inf) the
    device gives the same Inf or a NaN for a NaN"""
    ref, cells, nan_cells, volume, ab = reference(H, field, comp, lo, hi, nbins)
    assert P.cells.dtype == np.int64 and P.cells.shape == cells.shape and np.array_equal(P.cells, cells), (what, field, nbins, P.cells, cells)
    assert P.nan_cells == nan_cells, (what, field, nbins, P.nan_cells, nan_cells)
    assert np.array_equal(P["volume"].view(np.uint64), volume.view(np.uint64)), (what, field, nbins, P["volume"], volume)
    n = cells.sum(axis=0)
    worst = 0.0
    for g in SUM_GROUPS:
        got = group(P, g)
        assert got.shape == ref[g].shape, (what, g, got.shape, ref[g].shape)
        fin = np.isfinite(ref[g]) & np.isfinite(ab[g])
        with np.errstate(invalid="ignore"):
            same = (got == ref[g]) | (np.isnan(got) & np.isnan(ref[g]))
            bound = (n[None, :] + 8) * EPS * ab[g]
            diff = np.abs(got - ref[g])
            ok = np.where(fin, diff <= bound, same)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(fin & (bound > 0), diff / bound, 0.0))))
        bad = np.argwhere(~ok)
        assert bad.size == 0, (what, field, nbins, g, bad[:4], got[tuple(bad[0])], ref[g][tuple(bad[0])], bound[tuple(bad[0])])
        assert (got[:, n == 0] == 0.0).all() and not np.signbit(got[:, n == 0]).any(), (what, g, "an empty slot is +0")
    print("%s %s[%d] %d bins: %d cells, %d NaN; the largest |device - numpy| / bound = %.3f" % (what, field, comp, nbins, int(n.sum()), nan_cells, worst))
    return ref, cells, nan_cells, volume, ab


def reference2(H, a1, a2):
    """vdn_pdf2 in numpy: cells (nlev, n1 + 2, n2 + 2), nan_cells (either value NaN), volume"""
    with np.errstate(invalid="ignore"):
        U, S, M = H.gather(H.u), H.gather(H.s), H.composite()
        Q1, Q2 = bin_field(H, U, S, a1[0], a1[1]), bin_field(H, U, S, a2[0], a2[1])
    shape = (a1[4] + 2, a2[4] + 2)
    cells, nan_cells, volume = np.zeros((H.nlev,) + shape, dtype=np.int64), 0, np.zeros(shape)
    for l in range(H.nlev):
        s1, s2 = slots(Q1[l][M[l]], a1[2], a1[3], a1[4]), slots(Q2[l][M[l]], a2[2], a2[3], a2[4])
        keep = (s1 >= 0) & (s2 >= 0)
        nan_cells += int((~keep).sum())
        np.add.at(cells[l], (s1[keep], s2[keep]), 1)
        volume = volume + cells[l].astype(np.float64) * float(np.prod(H.dx[l]))
    return cells, nan_cells, volume


def pdf(H, field, comp, lo, hi, nbins):
    return H.pkg.advance.pdf(H.mla, H.u, H.s, H.dx, H.bct, field, comp, lo, hi, nbins)


def pdf2(H, a1, a2):
    return H.pkg.advance.pdf2(H.mla, H.u, H.s, H.dx, H.bct, a1[0], a1[1], a1[2], a1[3], a1[4], a2[0], a2[1], a2[2], a2[3], a2[4])


def all_bits(P):
    """every figure of a Pdf object as its 64-bit pattern: the rows, the counts, the NaN cells"""
    return np.concatenate([np.ascontiguousarray(P.rows).view(np.uint64).ravel(), P.cells.astype(np.uint64).ravel(), np.array([P.nan_cells], dtype=np.uint64)])


def all_bits2(P):
    return np.concatenate([P.cells.astype(np.uint64).ravel(), np.ascontiguousarray(P.volume).view(np.uint64).ravel(), np.array([P.nan_cells], dtype=np.uint64)])


def rank_figures(H):
    """what the two-call and the rank tests compare: every axis of RANK_AXES twice, the pair once (the vorticity's ghost cells are filled by make_vorticity first)"""
    vorticity(H)
    out = {}
    for i, ax in enumerate(RANK_AXES):
        out["axis%d" % i] = all_bits(pdf(H, *ax))
        out["again%d" % i] = all_bits(pdf(H, *ax))
    out["pair"] = all_bits2(pdf2(H, *RANK_PAIR))
    return out


def main():
    ranks, nranks = [int(r) for r in sys.argv[1].split(",")], int(sys.argv[2])
    from tests._rank_threads import run_ranks
    run_ranks(ranks, lambda rank, pkg: one_rank(rank, nranks, pkg), os.path.dirname(sys.argv[4]))


def one_rank(rank, nranks, pkg):
    idfile, outprefix = sys.argv[3], sys.argv[4]
    prm = pkg.capi.default_params(nscal=3)
    comm_id = rendezvous(pkg.boxlib, prm, rank, nranks, idfile)
    from tests._diagnostics_worker import Hier
    H = Hier(pkg, AMR3[0], AMR3[1], nscal=3, seed=7, rank=rank, nranks=nranks, comm_id=comm_id)
    H.dx = [[2.0 ** -((3, 2, 4)[d] + l) for d in range(H.dm)] for l in range(H.nlev)]
    save_rank(outprefix, rank, rank_figures(H))
    H.close()
    if nranks > 1:
        pkg.boxlib.comm_finalize()


if __name__ == "__main__":
    main()
