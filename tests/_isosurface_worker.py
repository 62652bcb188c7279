"""Isosurfaces (vdn_isosurface): the definitions of include/varden_amd.h restated in numpy float64 -- node means with the face-value rule, the six Kuhn tetrahedra, the
crossings, the triangles in output order, the per-term area, area vector and volume -- on the grids of tests/_profiles_worker.py, and one or several ranks (threads,
tests/_rank_threads.py) of the rank-independence test on ONE GPU (tests/test_isosurface_gpu.py::test_ranks_give_identical_bits).  The orientation of a triangle is
NOT taken from the library's table: restate() builds every case once on a unit cube with values +-1 and turns the triangle so that (p1 - p0) x (p2 - p0) has a positive
component along -grad q of the tetrahedron's linear interpolant.
argv: rank[,rank...] nranks idfile outprefix"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests._diagnostics_worker import Hier  # noqa: E402
from tests._profiles_worker import AMR3, EPS  # noqa: E402
from tests.children import rendezvous, save_rank  # noqa: E402

ORDERS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
OTHERS = {0: (1, 2, 3), 1: (0, 3, 2), 2: (0, 1, 3), 3: (0, 2, 1)}
WALLS, INLET_X, PERIODIC_Y = [[15, 15]] * 3, [[11, 12], [15, 15], [15, 15]], [[15, 15], [-1, -1], [15, 15]]
COUNTS = ("ntri", "cut_cells", "nonfinite_cells")
STRUCT = ("ntri", "ntri_lev", "cut_cells", "cut_cells_lev", "nonfinite_cells", "written", "area", "area_lev", "area_vec", "volume_above", "volume")
RANK_ISO = 0.125
NFIG, WRITTEN = 22, 11


def ext_dir(phys, bccomp, d, dm=3, nscal=2):
    """whether the adv boundary type of component bccomp at a face of physical type phys, direction d, is EXT_DIR (define_bc_tower): an inlet gives the velocity and
    the scalars a value on the face, an outlet (and a symmetry face) the pressure, a no-slip wall the velocity, a slip wall the normal velocity"""
    return (phys == 11 and bccomp < dm + nscal) or (phys in (12, 13) and bccomp == dm + nscal) or (phys == 15 and bccomp < dm) or (phys == 14 and bccomp == d)


def hier(pkg, nbase, boxes, dx0=(2.0 ** -3, 2.0 ** -2, 2.0 ** -4), **kw):
    """Hier with one ghost layer of s and spacings that differ per direction and are powers of two, halved per level"""
    H = Hier(pkg, nbase, boxes, ng_s=1, plant_zeros=False, **kw)
    H.dx = [[dx0[d] / (1 << l) for d in range(3)] for l in range(H.nlev)]
    return H


def random_field(H, seed, periodic=()):
    """per level one array over the level's GROWN domain (one ghost layer): seeded random multiples of 1/8 in [-1, 1], so node values (multiples of 1/64) equal an iso
    value that is one somewhere; along a periodic direction the ghost layers hold the opposite side's bits"""
    A = []
    for l in range(H.nlev):
        rng = np.random.default_rng(7919 * seed + l)
        a = np.round(rng.uniform(-1.0, 1.0, tuple(n + 2 for n in H.n[l])) * 8.0) / 8.0
        for d in periodic:
            lo, hi = [slice(None)] * 3, [slice(None)] * 3
            lo[d], hi[d] = 0, -2
            a[tuple(lo)] = a[tuple(hi)]
            lo[d], hi[d] = -1, 1
            a[tuple(lo)] = a[tuple(hi)]
        A.append(a)
    return A


def write_field(H, A, comp=0):
    """component comp of H.s, valid AND ghost cells of every local box, from the grown arrays: the test writes every cell the call reads"""
    for l, mf in enumerate(H.s):
        for i in range(mf.nfabs()):
            lo, hi = mf.get_box(i)
            f = mf.to_numpy(i)
            f[..., comp] = A[l][tuple(slice(lo[d], hi[d] + 3) for d in range(3))]
            mf.from_numpy(f, i)


def isosurface(H, iso, bccomp=3, comp=0, triangles=True):
    return H.pkg.advance.isosurface(H.mla, H.s, comp, bccomp, H.dx, H.bct, iso, triangles=triangles)


def node_values(a, flo, fhi):
    """the nodes of a level from its grown cell array: pairwise means along x, then y, then z; on a face with a face value the ghost cell alone"""
    for d in range(3):
        n = a.shape[d] - 2
        lo, hi = np.take(a, np.arange(0, n + 1), axis=d), np.take(a, np.arange(1, n + 2), axis=d)
        m = 0.5 * lo + 0.5 * hi
        first, last = [slice(None)] * 3, [slice(None)] * 3
        first[d], last[d] = 0, n
        if flo[d]:
            m[tuple(first)] = lo[tuple(first)]
        if fhi[d]:
            m[tuple(last)] = hi[tuple(last)]
        a = m
    return a


def _tet_case(n, m, qv, X, iso, vtet):
    """tetrahedron n, mask m, for a batch of cells: qv (cells, 4) its vertex values, X (cells, 4, 3) its vertex positions.  Returns the triangles as stated (a list of
    (cells, 3, 3), not yet turned) and the volume above (cells,)"""
    def cross(A, B):                                   # from the not-above vertex A to the above vertex B
        t = (iso - qv[:, A]) / (qv[:, B] - qv[:, A])
        return X[:, A] + t[:, None] * (X[:, B] - X[:, A]), t
    above = [v for v in range(4) if (m >> v) & 1]
    below = [v for v in range(4) if not (m >> v) & 1]
    if len(above) == 1:
        L = above[0]
        (p1, t1), (p2, t2), (p3, t3) = [cross(o, L) for o in OTHERS[L]]
        return [np.stack([p1, p2, p3], axis=1)], ((vtet * (1.0 - t1)) * (1.0 - t2)) * (1.0 - t3)
    if len(above) == 3:
        L = below[0]
        (p1, t1), (p2, t2), (p3, t3) = [cross(L, o) for o in OTHERS[L]]
        return [np.stack([p1, p2, p3], axis=1)], vtet - ((vtet * t1) * t2) * t3
    (A1, A2), (B1, B2) = above, below
    (p11, t11), (p12, t12), (p21, t21), (p22, t22) = cross(B1, A1), cross(B1, A2), cross(B2, A1), cross(B2, A2)
    a, b, c, d = 1.0 - t11, 1.0 - t21, 1.0 - t12, 1.0 - t22
    return [np.stack([p11, p12, p22], axis=1), np.stack([p11, p22, p21], axis=1)], (((vtet * a) * b) + (((vtet * t11) * b) * c)) + (((vtet * t21) * c) * d)


def _tri_cross(T):
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def _corners(n):
    o = ORDERS[n]
    return (0, 1 << o[0], (1 << o[0]) | (1 << o[1]), 7)


_TURN = {}


def turned(n, m):
    """per triangle of case (n, m): whether its last two vertices change places -- from the RULE: the case on the unit cube with values +-1, the normal against the
    gradient of the tetrahedron's linear interpolant (its edges v0 v1, v1 v2, v2 v3 run along the axes of its order)"""
    if (n, m) not in _TURN:
        c, o = _corners(n), ORDERS[n]
        qv = np.array([[1.0 if (m >> v) & 1 else -1.0 for v in range(4)]])
        X = np.array([[[float((c[v] >> d) & 1) for d in range(3)] for v in range(4)]])
        g = np.zeros(3)
        for e in range(3):
            g[o[e]] = qv[0, e + 1] - qv[0, e]
        tris, _ = _tet_case(n, m, qv, X, 0.0, 1.0 / 6.0)
        dots = [float(_tri_cross(T)[0] @ -g) for T in tris]
        assert all(abs(v) > 0.01 for v in dots), (n, m, dots)
        _TURN[n, m] = [v < 0.0 for v in dots]
    return _TURN[n, m]


def restate(H, A, iso, bccomp=3, phys=WALLS):
    """vdn_isosurface in numpy: a dict with tri (ntri, 3, 3) and level in output order, the counts per level, nonfinite_cells, volume, and the TERMS of the sums in
    float64 exactly as stated -- area and area_vec per triangle, volume above per tetrahedron -- with the level of each"""
    M = H.composite()
    flo = [ext_dir(phys[d][0], bccomp, d, 3, H.nscal) for d in range(3)]
    fhi = [ext_dir(phys[d][1], bccomp, d, 3, H.nscal) for d in range(3)]
    R = dict(tri=[], level=[], ntri_lev=[], cut_cells_lev=[], nonfinite_cells=0, volume=0.0, vol_terms=[], cell_of=[])
    first_cell = 0
    for l in range(H.nlev):
        N = node_values(A[l], flo, fhi)
        dx = np.array(H.dx[l])
        vol = (H.dx[l][0] * H.dx[l][1]) * H.dx[l][2]
        vtet = vol / 6.0
        idx = []
        for lo, hi in H.boxes[l]:                      # level, global box, then k, j, i with i fastest
            sub = M[l][tuple(slice(lo[d], hi[d] + 1) for d in range(3))]
            idx.append(np.argwhere(sub.transpose(2, 1, 0))[:, ::-1] + np.array(lo))
        idx = np.concatenate(idx)
        q = np.stack([N[idx[:, 0] + (c & 1), idx[:, 1] + ((c >> 1) & 1), idx[:, 2] + ((c >> 2) & 1)] for c in range(8)], axis=1)
        fin = np.isfinite(q).all(axis=1)
        R["nonfinite_cells"] += int((~fin).sum())
        R["volume"] = R["volume"] + float(int(fin.sum())) * vol
        rank = np.arange(len(idx))[fin]
        idx, q = idx[fin], q[fin]
        xlo, xhi = idx * dx, (idx + 1) * dx
        tris, keys, ntri_cell = [], [], np.zeros(len(idx), dtype=np.int64)
        for n in range(6):
            c = _corners(n)
            qv = q[:, c]
            X = np.stack([np.where([(c[v] >> d) & 1 for d in range(3)], xhi, xlo) for v in range(4)], axis=1)
            with np.errstate(invalid="ignore"):
                mask = ((qv > iso) * (1 << np.arange(4))).sum(axis=1)
            R["vol_terms"].append(np.full(int((mask == 15).sum()), vtet))
            for m in range(1, 15):
                sel = np.nonzero(mask == m)[0]
                if sel.size == 0:
                    continue
                T, v = _tet_case(n, m, qv[sel], X[sel], iso, vtet)
                R["vol_terms"].append(v)
                for k, (t, turn) in enumerate(zip(T, turned(n, m))):
                    tris.append(t[:, [0, 2, 1]] if turn else t)
                    keys.append(np.stack([rank[sel], np.full(sel.size, n), np.full(sel.size, k)], axis=1))
                ntri_cell[sel] += len(T)
        if tris:
            tris, keys = np.concatenate(tris), np.concatenate(keys)
            order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
            R["tri"].append(tris[order])
            R["cell_of"].append(first_cell + keys[order, 0])
        first_cell += len(fin)
        R["ntri_lev"].append(int(ntri_cell.sum()))
        R["cut_cells_lev"].append(int((ntri_cell > 0).sum()))
        R["level"].append(np.full(R["ntri_lev"][-1], l, dtype=np.uint8))
    R["tri"] = np.concatenate(R["tri"]) if R["tri"] else np.zeros((0, 3, 3))
    R["cell_of"] = np.concatenate(R["cell_of"]) if R["cell_of"] else np.zeros(0, dtype=np.int64)
    R["level"], R["vol_terms"] = np.concatenate(R["level"]), np.concatenate(R["vol_terms"])
    R["ntri"], R["cut_cells"] = sum(R["ntri_lev"]), sum(R["cut_cells_lev"])
    cr = _tri_cross(R["tri"])
    R["area_terms"] = 0.5 * np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
    R["av_terms"] = 0.5 * cr
    return R


def canonical(tri):
    """every triangle turned (cyclically: the orientation stays) to its lexicographically smallest rotation, smallest vertex first"""
    out = np.array(tri, dtype=np.float64)
    for t in range(out.shape[0]):
        rot = [tuple(np.roll(out[t], -r, axis=0).ravel()) for r in range(3)]
        out[t] = np.array(min(rot)).reshape(3, 3)
    return out


def wide_sum(t):
    """(the sum of the terms, the sum of their magnitudes) in numpy.longdouble"""
    t = np.asarray(t, dtype=np.longdouble)
    return t.sum(), np.abs(t).sum()


def sum_bound(n, abs_sum, c=1):
    """(n + c) 2^-53 sum |term|: a sum of n terms in any order or tree makes n - 1 roundings; c counts the roundings beside them.  Against restate() the terms
    themselves are the device's bits -- the same float64 expression in the same order, no contraction, division and square root correctly rounded on both sides --
    so c = 1: the conversion of the wide sum to double"""
    return float((n + c) * EPS * abs_sum)


def check(I, R, what=""):
    """an Iso object against restate(): the counts exactly, the triangles bit for bit in output order (each turned to its smallest vertex first), the levels, and the
    sums within sum_bound of sums formed in numpy.longdouble"""
    assert I.ntri == R["ntri"] and I.ntri_lev == R["ntri_lev"], (what, I.ntri, I.ntri_lev, R["ntri"], R["ntri_lev"])
    assert I.cut_cells == R["cut_cells"] and I.cut_cells_lev == R["cut_cells_lev"], (what, I.cut_cells_lev, R["cut_cells_lev"])
    assert I.nonfinite_cells == R["nonfinite_cells"], (what, I.nonfinite_cells, R["nonfinite_cells"])
    assert np.array([I.volume]).view(np.uint64)[0] == np.array([R["volume"]]).view(np.uint64)[0], (what, I.volume, R["volume"])
    worst = 0.0
    if I.tri is not None:
        assert I.written == I.ntri and I.tri.shape == (I.ntri, 3, 3) and I.level.dtype == np.uint8 and np.array_equal(I.level, R["level"]), what
        got, want = canonical(I.tri), canonical(R["tri"])
        same = (got.view(np.uint64) == want.view(np.uint64)).reshape(-1, 9).all(axis=1)
        # cell by cell: the first triangle that differs names its cell
        assert same.all(), (what, "triangle %d (cell %d in output order)" % (int(np.argmin(same)), int(R["cell_of"][np.argmin(same)])), got[np.argmin(same)], want[np.argmin(same)])
        assert not np.signbit(I.tri).any(), what
    figures = [("area", I.area, R["area_terms"]), ("volume_above", I.volume_above, R["vol_terms"])]
    figures += [("area_vec[%d]" % d, I.area_vec[d], R["av_terms"][:, d]) for d in range(3)]
    figures += [("area_lev[%d]" % l, I.area_lev[l], R["area_terms"][R["level"] == l]) for l in range(len(R["ntri_lev"]))]
    for name, got, terms in figures:
        want, ab = wide_sum(terms)
        bound = sum_bound(len(terms), ab)
        diff = abs(float(np.longdouble(got) - want))
        print("%s %s: device %.17e numpy %.17e |diff| %.3e bound %.3e (%d terms)" % (what, name, got, float(want), diff, bound, len(terms)))
        assert diff <= bound, (what, name, got, float(want), diff, bound)
        worst = max(worst, diff / bound if bound > 0 else 0.0)
    return worst


def all_bits(I):
    """every figure of an Iso object as its 64-bit pattern: the struct's members in order (NFIG of them: the per-level lists filled up to four entries; `written`
    is entry WRITTEN), then the triangles and their levels"""
    out = []
    for name in STRUCT:
        v = getattr(I, name)
        if name.endswith("_lev"):
            v = list(v) + [type(v[0])(0)] * (4 - len(v))
        for x in (v if isinstance(v, list) else [v]):
            out.append(np.array([x], dtype=np.int64).view(np.uint64)[0] if isinstance(x, int) else np.array([x], dtype=np.float64).view(np.uint64)[0])
    parts = [np.array(out, dtype=np.uint64)]
    if I.tri is not None:
        parts += [np.ascontiguousarray(I.tri).view(np.uint64).ravel(), I.level.astype(np.uint64)]
    return np.concatenate(parts)


def rank_figures(H):
    """what the two-call and the rank tests compare: the surface of the random field on AMR3 with face values on every wall (bccomp 0), twice, and the counts alone"""
    write_field(H, random_field(H, 5))
    return dict(iso=all_bits(isosurface(H, RANK_ISO, bccomp=0)), again=all_bits(isosurface(H, RANK_ISO, bccomp=0)),
                counts=all_bits(isosurface(H, RANK_ISO, bccomp=0, triangles=False)))


def main():
    ranks, nranks = [int(r) for r in sys.argv[1].split(",")], int(sys.argv[2])
    from tests._rank_threads import run_ranks
    run_ranks(ranks, lambda rank, pkg: one_rank(rank, nranks, pkg), os.path.dirname(sys.argv[4]))


def one_rank(rank, nranks, pkg):
    idfile, outprefix = sys.argv[3], sys.argv[4]
    prm = pkg.capi.default_params(nscal=2)
    comm_id = rendezvous(pkg.boxlib, prm, rank, nranks, idfile)
    H = hier(pkg, AMR3[0], AMR3[1], nscal=2, seed=7, rank=rank, nranks=nranks, comm_id=comm_id)
    save_rank(outprefix, rank, rank_figures(H))
    H.close()
    if nranks > 1:
        pkg.boxlib.comm_finalize()


if __name__ == "__main__":
    main()
