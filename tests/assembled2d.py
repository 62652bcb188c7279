"""The two elliptic systems of the dm = 2 path assembled independently of the solvers, after tests/assembled.py (which stays the 3-D module):

  * cell-centred: the five-point (alpha - div beta grad) phi = rh.  tests/assembled.py's cc_matrix on (n0, n1, 1) cells with Neumann z-faces and a zero
    z-coefficient IS that system: one cell along z has no interior z-face and a Neumann face carries nothing (cc_matrix5 below; five_point is the same
    matrix written out by hand, the check of that sentence in tests/test_assembled_2d_cpu.py);
  * nodal: the Q1 stiffness matrix of cell-constant sigma assembled ELEMENT BY ELEMENT from kron(M1y, K1x) + kron(K1y, M1x), the load int u . grad N,
    everything scaled by 1/(hx hy); walls are natural boundaries, outflow nodes are Dirichlet, periodic nodes are identified -- asm.NodalLevel with
    the z factor dropped.  Its weights per unit sigma and element are 2(fx + fy), -2fx + fy, fx - 2fy, -(fx + fy) with f = 1/(6 h^2).
"""
import itertools

import numpy as np

from tests import assembled as asm

PER, INT, DIR, NEU = asm.PER, asm.INT, asm.DIR, asm.NEU


def smooth2(shape, h, seed, lo=(0, 0), off=0.5):
    """a smooth field of a few Fourier modes on shape[0] x shape[1] points at (index + lo + off) h"""
    rng = np.random.default_rng(seed)
    X, Y = np.meshgrid(*[(np.arange(shape[d]) + lo[d] + off) * h[d] for d in range(2)], indexing="ij")
    f = np.zeros(shape)
    for _ in range(4):
        k = rng.integers(1, 4, size=2); ph = rng.uniform(0, 2 * np.pi, size=2)
        f += rng.uniform(-1, 1) * np.sin(2 * np.pi * k[0] * X + ph[0]) * np.sin(2 * np.pi * k[1] * Y + ph[1])
    return f


def cc_matrix5(n, dx, bx, by, ell2, alpha=None):
    """n = (n0, n1); bx: (n0 + 1, n1), by: (n0, n1 + 1) face coefficients; ell2[d][side]; alpha: (n0, n1) or None.  Unknowns x fastest."""
    n0, n1 = int(n[0]), int(n[1])
    beta = [np.asarray(bx).reshape(n0 + 1, n1, 1), np.asarray(by).reshape(n0, n1 + 1, 1), np.zeros((n0, n1, 2))]
    return asm.cc_matrix((n0, n1, 1), [dx[0], dx[1], 1.0], beta, [list(ell2[0]), list(ell2[1]), [NEU, NEU]],
                         None if alpha is None else np.asarray(alpha).reshape(n0, n1, 1))


def five_point(n, dx, bx, by, ell2, alpha=None):
    """the same matrix cell by cell, dense (small n only): each face of a cell adds b/h^2 (phi_cell - phi_neighbour); beyond a Neumann face nothing,
    beyond a homogeneous Dirichlet face phi_neighbour = -phi_cell (2 b/h^2 on the diagonal), beyond a periodic face the cell at the other end"""
    n0, n1 = n
    A = np.zeros((n0 * n1, n0 * n1))
    for j in range(n1):
        for i in range(n0):
            r = i + n0 * j
            for d, side, b in ((0, 0, bx[i, j]), (0, 1, bx[i + 1, j]), (1, 0, by[i, j]), (1, 1, by[i, j + 1])):
                q = [i, j]; q[d] += 1 if side else -1
                c = b / (dx[d] * dx[d])
                if 0 <= q[d] < n[d]:
                    A[r, r] += c; A[r, q[0] + n0 * q[1]] -= c
                elif ell2[d][side] == PER:
                    q[d] %= n[d]
                    A[r, r] += c; A[r, q[0] + n0 * q[1]] -= c
                elif ell2[d][side] == DIR:
                    A[r, r] += 2.0 * c
            if alpha is not None:
                A[r, r] += alpha[i, j]
    return A


def q1_element_matrices2(h):
    """4 x 4 stiffness of the rectangle hx x hy with unit sigma (corner a + 2 b at offset (a, b)), and the 4 x 2 matrix of the integrals of
    dN_corner/dx_d over the rectangle"""
    K1 = [np.array([[1.0, -1.0], [-1.0, 1.0]]) / h[d] for d in range(2)]
    M1 = [h[d] / 6.0 * np.array([[2.0, 1.0], [1.0, 2.0]]) for d in range(2)]
    Ke = np.kron(M1[1], K1[0]) + np.kron(K1[1], M1[0])
    G = np.zeros((4, 2))
    for b, a in itertools.product(range(2), repeat=2):
        o = (a, b)
        for d in range(2):
            G[a + 2 * b, d] = (1.0 if o[d] else -1.0) * h[1 - d] / 2.0
    return Ke, G


class NodalLevel2:
    """nodes 0..n[d] of a box of n0 x n1 cells; a periodic direction identifies node n[d] with node 0.  stiffness: K in the energy form (unscaled);
    load(u): int u . grad N of a cell-constant vector field; both take 1/vol to become the solver's equations"""

    def __init__(self, n, dx, per=(0, 0)):
        self.n, self.dx, self.per = tuple(int(x) for x in n[:2]), tuple(float(x) for x in dx[:2]), tuple(int(x) for x in per[:2])
        self.nn = tuple(self.n[d] + (0 if self.per[d] else 1) for d in range(2))       # unique nodes
        self.N = self.nn[0] * self.nn[1]
        self.Ke, self.G = q1_element_matrices2(self.dx)
        self.vol = self.dx[0] * self.dx[1]
        ci = np.meshgrid(*[np.arange(self.n[d]) for d in range(2)], indexing="ij")
        self.corner = []
        for b, a in itertools.product(range(2), repeat=2):
            q = [ci[0] + a, ci[1] + b]
            for d in range(2):
                if self.per[d]:
                    q[d] = q[d] % self.n[d]
            self.corner.append((a + 2 * b, q[0] + self.nn[0] * q[1]))
        self.corner.sort(key=lambda t: t[0])

    def stiffness(self, sigma):
        acc = asm._coo()
        for a, na in self.corner:
            for b, nb in self.corner:
                acc[0].append(na); acc[1].append(nb); acc[2].append(sigma * self.Ke[a, b])
        return asm._csr(acc, (self.N, self.N))

    def load(self, u):
        """u: (n0, n1, 2) cell values"""
        w = np.zeros(self.N)
        for a, na in self.corner:
            for d in range(2):
                np.add.at(w, na.ravel(), (u[..., d] * self.G[a, d]).ravel())
        return w

    def to_grid(self, x):
        """unique-node vector -> array on nodes 0..n[d] (images filled)"""
        g = np.asarray(x).reshape(self.nn, order="F")
        for d in range(2):
            if self.per[d]:
                g = np.concatenate([g, np.take(g, [0], axis=d)], axis=d)
        return g

    def from_grid(self, g):
        return np.asarray(g)[:self.nn[0], :self.nn[1]].ravel(order="F")

    def dirichlet_mask(self, ellbc):
        m = np.zeros(self.nn, dtype=bool)
        for d in range(2):
            if ellbc[d][0] == DIR:
                sl = [slice(None)] * 2; sl[d] = 0; m[tuple(sl)] = True
            if ellbc[d][1] == DIR:
                sl = [slice(None)] * 2; sl[d] = self.nn[d] - 1; m[tuple(sl)] = True
        return m.ravel(order="F")


# ---- the test systems of tests/test_bottom_solver_2d_gpu.py and tests/test_assembled_2d_cpu.py: data, matrix, direct solution ----
SHAPES = [(70, 66), (44, 52), (24, 24), (40, 12)]
ELL2 = {"walls": [[NEU, NEU], [NEU, NEU]], "inout": [[NEU, DIR], [NEU, NEU]], "periodic": [[PER, PER], [PER, PER]], "periodic-x": [[PER, PER], [NEU, NEU]]}


def cc_data(n, ell2, with_alpha=False):
    """face coefficients as mk_mac_coeffs makes them from a smooth positive density (periodic sides wrap), a right-hand side (zero mean where the system
    is singular), alpha: a smooth positive rho / (mu dt)-like cell field"""
    dx = [1.0 / max(n)] * 2
    rho = 2.0 + 0.45 * smooth2((n[0] + 2, n[1] + 2), dx, 21, lo=(-1, -1))
    for d in range(2):
        if ell2[d][0] == PER:
            g, s = [slice(None)] * 2, [slice(None)] * 2
            g[d], s[d] = 0, -2; rho[tuple(g)] = rho[tuple(s)]
            g[d], s[d] = -1, 1; rho[tuple(g)] = rho[tuple(s)]
    bx = 2.0 / (rho[1:, 1:-1] + rho[:-1, 1:-1])
    by = 2.0 / (rho[1:-1, 1:] + rho[1:-1, :-1])
    rng = np.random.default_rng(5)
    b = smooth2(n, dx, 7) + 0.1 * rng.standard_normal(n)
    alpha = (rho[1:-1, 1:-1] * 40.0).copy() if with_alpha else None
    singular = alpha is None and not any(ell2[d][s] == DIR for d in range(2) for s in range(2))
    if singular:
        b -= b.mean()
    return dx, bx, by, b, alpha, singular


def cc_system(n, bcname, with_alpha=False):
    ell2 = ELL2[bcname]
    dx, bx, by, b, alpha, singular = cc_data(n, ell2, with_alpha)
    A = cc_matrix5(n, dx, bx, by, ell2, alpha)
    xd, lam = asm.solve_maybe_singular(A, b.ravel(order="F"), np.ones(A.shape[0]) if singular else None)
    if singular:
        xd = xd - xd.mean()
    for a in (bx, by, b, xd) + (() if alpha is None else (alpha,)):
        a.setflags(write=False)
    return dict(A=A, dx=dx, bx=bx, by=by, b=b, alpha=alpha, xd=xd, lam=lam, singular=singular, ell2=ell2)


def nd_system(n, bcname):
    ell2 = ELL2[bcname]
    per = tuple(1 if ell2[d][0] == PER else 0 for d in range(2))
    dx = [1.0 / max(n)] * 2
    sig = 1.0 / (2.0 + 0.45 * smooth2(n, dx, 5))
    u = np.stack([smooth2(n, dx, 11 + c) for c in range(2)], axis=-1)
    NL = NodalLevel2(n, dx, per)
    K = NL.stiffness(sig) / NL.vol
    w = NL.load(u) / NL.vol
    free = ~NL.dirichlet_mask(ell2)
    singular = bool(free.all())
    yd, lam = asm.solve_maybe_singular(K[free][:, free], w[free], np.ones(int(free.sum())) if singular else None)
    if singular:
        yd = yd - yd.mean()
    for a in (sig, u, yd):
        a.setflags(write=False)
    return dict(NL=NL, K=K, w=w, dx=dx, sig=sig, u=u, free=free, yd=yd, lam=lam, singular=singular, ell2=ell2, per=per)
