"""Run diagnostics (vdn_diagnostics): the hierarchies with random fields the tests run it on, the numpy reference over the composite grid, and one or several
ranks (threads, tests/_rank_threads.py) of the rank-independence test on ONE GPU (tests/test_diagnostics_gpu.py::test_ranks_give_identical_bits).
argv: rank[,rank...] nranks idfile outprefix case"""
import math
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.children import rendezvous, save_rank  # noqa: E402

WALLS = [[15, 15]] * 3
FIELDS = ("cells", "cells_lev", "nonfinite", "volume", "volume_lev", "sum_s", "momentum", "kinetic", "enstrophy",
          "s_min", "s_max", "u_min", "u_max", "magvel_max", "vort_min", "vort_max")
SUMS = ("volume", "volume_lev", "sum_s", "momentum", "kinetic", "enstrophy")

# fixed hierarchies (boxes per level, each level in its own index space).  amr2: a 16^3 base in two boxes, one fine box on the domain wall x = 0, one whose low
# x face lies on the coarse boxes' common edge (coarse x = 8); amr3: a 32^3 base in eight boxes, two boxes on level 1 (one on the wall), one on level 2
CASES = {
    "amr2": (16, [[((0, 0, 0), (7, 15, 15)), ((8, 0, 0), (15, 15, 15))],
                  [((0, 8, 8), (15, 23, 19)), ((16, 8, 4), (27, 19, 23))]]),
    "amr3": (32, [[((16 * i, 16 * j, 16 * k), (16 * i + 15, 16 * j + 15, 16 * k + 15)) for k in range(2) for j in range(2) for i in range(2)],
                  [((16, 16, 16), (47, 47, 47)), ((0, 16, 20), (15, 31, 43))],
                  [((40, 40, 40), (87, 75, 83))]]),
}


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def okey(a):
    """the order-preserving 64-bit image of doubles (csrc/vdn_dev.h: key_of): -0 sorts below +0"""
    b = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def from_key(k):
    k = int(k)
    b = (k & 0x7FFFFFFFFFFFFFFF) if k >> 63 else (~k & 0xFFFFFFFFFFFFFFFF)
    return struct.unpack("<d", struct.pack("<Q", b))[0]


class Hier:
    """a hierarchy of box lists with random u (dm components, ng_u ghost layers) and s (nscal, ng_s): every level's fields are cut out of one random array over the
    level's grown domain, so ghost cells agree with their neighbours' valid cells and do not depend on the ranks.  Cells are dx = (1, 2, 1/2) / n: the domain's volume
    is 1 (dm = 3) or 2 (dm = 2).  The last scalar is >= 0 but for one -0.0, velocity component 1 is <= 0 but for one -0.0 and one +0.0, on the finest level."""

    def __init__(self, pkg, nbase, boxes, phys=WALLS, nscal=2, dm=3, seed=0, rank=0, nranks=1, comm_id=None, ng_u=1, ng_s=2, nan_ghosts=False, plant_zeros=True):
        bl = self.bl = pkg.boxlib
        self.pkg, self.dm, self.nscal, self.rank = pkg, dm, nscal, rank
        self.prm = pkg.capi.default_params(dm=dm, nscal=nscal)
        bl.initialize(self.prm, rank, nranks, 0)
        if comm_id is not None:
            bl.comm_init(comm_id)
        nb = (nbase,) * dm if isinstance(nbase, int) else tuple(nbase)
        self.nlev = NL = len(boxes)
        self.boxes = [[(tuple(lo), tuple(hi)) for lo, hi in lev] for lev in boxes]
        self.n = [tuple((nb[d] << l) if d < dm else 1 for d in range(3)) for l in range(NL)]
        self.owner = [[i % nranks for i in range(len(lev))] for lev in self.boxes]
        self.phys = [list(phys[d]) if d < dm else [0, 0] for d in range(3)]
        self.mla = bl.MLLayout([((0, 0, 0), tuple(x - 1 for x in self.n[l])) for l in range(NL)], self.boxes, owner=self.owner, rr=[(2, 2, 2)] * (NL - 1),
                               pmask=[1 if self.phys[d][0] == -1 else 0 for d in range(3)])
        self.bct = bl.BCTower(self.mla, self.phys)
        self.dx = [[(1.0, 2.0, 0.5)[d] / self.n[l][d] for d in range(dm)] for l in range(NL)]
        self.u, self.s = [], []
        for l in range(NL):
            rng = np.random.default_rng(1000 * seed + l)
            full = {}
            for name, nc, ng in (("u", dm, ng_u), ("s", nscal, ng_s)):
                g = tuple(ng if d < dm else 0 for d in range(3))
                a = rng.uniform(-1.0, 1.0, tuple(self.n[l][d] + 2 * g[d] for d in range(3)) + (nc,))
                if plant_zeros:
                    if name == "s":
                        a[..., nc - 1] = np.abs(a[..., nc - 1]) + 1e-3
                    else:
                        a[..., 1] = -np.abs(a[..., 1]) - 1e-3
                    if l == NL - 1:
                        lo = self.boxes[l][0][0]
                        c = tuple(lo[d] + g[d] for d in range(3))
                        if name == "s":
                            a[c + (nc - 1,)] = -0.0
                        else:
                            a[c + (1,)] = 0.0
                            a[(c[0] + 1, c[1], c[2], 1)] = -0.0
                full[name] = (a, g, ng)
            mfs = {}
            for name, nc, ng in (("u", dm, ng_u), ("s", nscal, ng_s)):
                a, g, _ = full[name]
                mf = bl.MultiFab(self.mla, l, nc, ng)
                for i in range(mf.nfabs()):
                    lo, hi = mf.get_box(i)
                    f = np.array(a[tuple(slice(lo[d], hi[d] + 1 + 2 * g[d]) for d in range(3))], order="F")
                    if nan_ghosts:
                        v = np.array(f[tuple(slice(g[d], f.shape[d] - g[d]) for d in range(3))])
                        f[...] = np.nan
                        f[tuple(slice(g[d], f.shape[d] - g[d]) for d in range(3))] = v
                    mf.from_numpy(f, i)
                mfs[name] = mf
            self.u.append(mfs["u"])
            self.s.append(mfs["s"])

    def diagnostics(self, vort=True):
        return self.pkg.advance.diagnostics(self.mla, self.u, self.s, self.dx, self.bct, vort=vort)

    def gather(self, mfs):
        """per level: the valid cells of every (local) box of to_numpy() in one array over the level's domain, NaN elsewhere"""
        out = []
        for l, mf in enumerate(mfs):
            a = np.full(self.n[l] + (mf.nc,), np.nan)
            for i in range(mf.nfabs()):
                lo, hi = mf.get_box(i)
                f = mf.to_numpy(i)
                g = [mf.ng if f.shape[d] > hi[d] - lo[d] + 1 else 0 for d in range(3)]
                a[tuple(slice(lo[d], hi[d] + 1) for d in range(3))] = f[tuple(slice(g[d], f.shape[d] - g[d]) for d in range(3))]
            out.append(a)
        return out

    def composite(self):
        """per level: True on the valid cells of the level that no box of the next level covers"""
        inbox = []
        for l in range(self.nlev):
            m = np.zeros(self.n[l], dtype=bool)
            for lo, hi in self.boxes[l]:
                m[tuple(slice(lo[d], hi[d] + 1) for d in range(3))] = True
            inbox.append(m)
        out = []
        for l in range(self.nlev):
            m = inbox[l].copy()
            if l + 1 < self.nlev:
                for lo, hi in self.boxes[l + 1]:
                    m[tuple(slice(lo[d] // 2, hi[d] // 2 + 1) for d in range(3))] = False
            out.append(m)
        return out

    def close(self):
        for m in self.u + self.s:
            m.destroy()
        self.bct.destroy()
        self.mla.destroy()


def reference(H, U, S, W=None):
    """numpy over the composite grid.  U, S: per level arrays over the level's domain (Hier.gather); W: the same for the vorticity (component 0), or None.
    Returns (figures, bound): figures as advance.diagnostics names them, sums added exactly (math.fsum) from the terms term = value * cell volume; bound[name]: the
    rounding bound of adding those terms in any order, ncells * 2^-53 * sum |term| (a list where the figure is one)"""
    dm, ns = H.dm, H.nscal
    M = H.composite()
    vol = [float(np.prod(H.dx[l])) for l in range(H.nlev)]
    ncell = int(sum(m.sum() for m in M))
    eps = 2.0 ** -53
    R = dict(cells=ncell, cells_lev=[int(m.sum()) for m in M], volume_lev=[vol[l] * int(M[l].sum()) for l in range(H.nlev)])
    R["volume"] = math.fsum(R["volume_lev"])
    u = np.concatenate([U[l][M[l]] for l in range(H.nlev)])          # (cells, dm)
    s = np.concatenate([S[l][M[l]] for l in range(H.nlev)])
    dv = np.concatenate([np.full(int(M[l].sum()), vol[l]) for l in range(H.nlev)])
    R["nonfinite"] = int((~(np.isfinite(u).all(axis=1) & np.isfinite(s).all(axis=1))).sum())
    B = dict(volume=ncell * eps * R["volume"], volume_lev=[ncell * eps * v for v in R["volume_lev"]])

    def integral(terms):
        return math.fsum(terms), ncell * eps * math.fsum(np.abs(terms))
    for name, cols in (("sum_s", [s[:, c] * dv for c in range(ns)]), ("momentum", [s[:, 0] * u[:, d] * dv for d in range(dm)])):
        pairs = [integral(t) for t in cols]
        R[name], B[name] = [p[0] for p in pairs], [p[1] for p in pairs]
    R["kinetic"], B["kinetic"] = integral(0.5 * s[:, 0] * (u * u).sum(axis=1) * dv)
    R["s_min"], R["s_max"] = [from_key(okey(s[:, c]).min()) for c in range(ns)], [from_key(okey(s[:, c]).max()) for c in range(ns)]
    R["u_min"], R["u_max"] = [from_key(okey(u[:, d]).min()) for d in range(dm)], [from_key(okey(u[:, d]).max()) for d in range(dm)]
    q = u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]
    if dm == 3:
        q = q + u[:, 2] * u[:, 2]
    R["magvel_max"] = from_key(okey(np.sqrt(q)).max())
    if W is not None:
        w = np.concatenate([W[l][M[l]][:, 0] for l in range(H.nlev)])
        R["enstrophy"], B["enstrophy"] = integral(0.5 * w * w * dv)
        R["vort_min"], R["vort_max"] = from_key(okey(w).min()), from_key(okey(w).max())
    else:
        R["enstrophy"], B["enstrophy"], R["vort_min"], R["vort_max"] = 0.0, 0.0, 0.0, 0.0
    return R, B


def all_bits(d):
    """every figure of a diagnostics dict as its 64-bit pattern, in FIELDS order"""
    out = []
    for name in FIELDS:
        v = d[name]
        for x in (v if isinstance(v, list) else [v]):
            out.append(int(x) if name in ("cells", "cells_lev", "nonfinite") else bits(x))
    return np.array(out, dtype=np.uint64)


def main():
    ranks, nranks = [int(r) for r in sys.argv[1].split(",")], int(sys.argv[2])
    from tests._rank_threads import run_ranks
    run_ranks(ranks, lambda rank, pkg: one_rank(rank, nranks, pkg), os.path.dirname(sys.argv[4]))


def one_rank(rank, nranks, pkg):
    idfile, outprefix, case = sys.argv[3], sys.argv[4], sys.argv[5]
    prm = pkg.capi.default_params(nscal=3)
    comm_id = rendezvous(pkg.boxlib, prm, rank, nranks, idfile)
    nbase, boxes = CASES[case]
    H = Hier(pkg, nbase, boxes, nscal=3, seed=7, rank=rank, nranks=nranks, comm_id=comm_id)
    a = all_bits(H.diagnostics(vort=True))
    b = all_bits(H.diagnostics(vort=True))
    c = all_bits(H.diagnostics(vort=False))
    save_rank(outprefix, rank, {"bits": a, "again": b, "novort": c})
    H.close()
    if nranks > 1:
        pkg.boxlib.comm_finalize()


if __name__ == "__main__":
    main()
