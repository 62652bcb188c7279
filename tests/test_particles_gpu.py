"""Values at points (vdn_sample_points) and Lagrangian tracer particles (vdn_particles_*; varden_amd/csrc/particles.hip) against the numpy restatement of their
definitions (tests/_particles_worker.py): host level and interpolated values bit for bit on one level, in dm = 2 and on hierarchies; a linear field reproduced to
rounding; Heun's move bit for bit, and its geometry on flows whose pathlines are known; the same bits on one, two and four ranks; real runs whose fields do not
change when particles ride along; particle files; every refusal."""
import os

import numpy as np
import pytest

from tests._diagnostics_worker import CASES, WALLS, Hier
from tests._particles_worker import Grid, box_arrays, extdir_of, heun, lattice_points, locate, sample, second_velocity
from tests.children import launch_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INOUT = [[11, 12], [14, 14], [15, 15]]          # inflow / outflow along x, slip and no-slip walls
PERIODIC = [[-1, -1]] * 3
ODD = (16, [[((0, 0, 0), (7, 15, 15)), ((8, 0, 0), (15, 15, 15))], [((3, 5, 2), (12, 9, 10))]])      # a fine box aligned to nothing: block size 1


def _pkg():
    import varden_amd
    from varden_amd import advance, boxlib, capi  # noqa: F401
    return varden_amd


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def planted(G, boxes0):
    """points where the rules change: cell centres, the common face of the base boxes, the half cell at every domain face, the domain's corners, a point exactly on
    each high face"""
    dm, L, dx = G.dm, G.len, G.dx[0]
    mid = [0.37 * L[d] for d in range(dm)]
    pts = []
    for c in ((0, 0, 0), (3, 7, 5), (G.n[0][0] - 1, G.n[0][1] - 1, G.n[0][2] - 1)):                 # cell centres
        pts.append([(c[d] + 0.5) * dx[d] for d in range(dm)])
    xf = (boxes0[0][1][0] + 1) * dx[0]                                                              # the boxes' common face, and one ulp either side
    for x in (xf, np.nextafter(xf, 0.0), np.nextafter(xf, 2.0 * xf)):
        pts.append([x] + mid[1:])
    for d in range(dm):
        for f in (0.0, 0.2, 0.5, 0.7, 1.0):                                                         # the half cell at the low and at the high face
            for base in (0.0, L[d] - 0.5 * dx[d]):
                p = list(mid)
                p[d] = min(base + f * 0.5 * dx[d], L[d])
                pts.append(p)
        p = list(mid)
        p[d] = L[d]                                                                                 # exactly on the high face
        pts.append(p)
    for corner in range(1 << dm):
        pts.append([L[d] if (corner >> d) & 1 else 0.0 for d in range(dm)])
    a = np.zeros((len(pts), 3))
    a[:, :dm] = np.array(pts)
    return a


def check_sampling(pkg, H, what, seed=3, nrandom=4099, want_all_levels=True):
    """u (nc = 1 and dm), s (nscal components, bccomp = dm) at random and planted points: values and levels equal numpy's bit for bit, no point left out"""
    adv = pkg.advance
    G = Grid.of(H)
    x = np.concatenate([lattice_points(G, nrandom, seed), planted(G, H.boxes[0])])
    for name, mfs, comp, nc, bccomp in (("u1", H.u, 0, 1, 0), ("u", H.u, 0, H.dm, 0), ("u-last", H.u, H.dm - 1, 1, H.dm - 1), ("s", H.s, 0, H.nscal, H.dm)):
        val, lev = adv.sample_points(H.mla, mfs, x, H.dx, H.bct, comp=comp, nc=nc, bccomp=bccomp)
        ref, rlev = sample(G, box_arrays(G, mfs), extdir_of(H.bct, H.dm, bccomp, nc), x, nc, comp=comp)
        assert val.shape == ref.shape == (x.shape[0], nc)
        assert np.array_equal(lev, rlev), (what, name, np.nonzero(lev != rlev)[0][:8])
        assert (lev >= 0).all(), (what, name, "a point inside the domain has no host")
        bad = np.nonzero(u64(val) != u64(ref))
        assert bad[0].size == 0, (what, name, bad[0][:8], val[bad][:8], ref[bad][:8], x[bad[0][:8]])
        assert np.isfinite(val).all()
    census = [int((lev == l).sum()) for l in range(H.nlev)]
    print("%s: points per host level %s" % (what, census))
    if want_all_levels:
        assert all(c > 0 for c in census), (what, census)
    # outside the domain: level -1, value 0
    out = np.array([[-1e-300, 0.1, 0.1], [0.1, G.len[1] * (1 + 1e-15), 0.1], [np.nan, 0.1, 0.1], [np.inf, 0.1, 0.1]])
    val, lev = adv.sample_points(H.mla, H.u, out, H.dx, H.bct, comp=0, nc=H.dm, bccomp=0)
    assert (lev == -1).all() and (u64(val) == 0).all(), (what, lev, val)
    return census


@pytest.mark.parametrize("phys", [WALLS, INOUT, PERIODIC], ids=["walls", "inout", "periodic"])
def test_sampling_one_level(gpu, phys):
    pkg = _pkg()
    H = Hier(pkg, 16, [[((0, 0, 0), (7, 15, 15)), ((8, 0, 0), (15, 15, 15))]], phys=phys, nscal=4, seed=1, plant_zeros=False)
    try:
        check_sampling(pkg, H, "16^3")
        # the face-value weights are in play exactly where the tower says EXT_DIR: every component at a no-slip wall and at the inflow face, the normal one alone
        # at a slip wall, none at the outflow face
        ext = extdir_of(H.bct, 3, 0, 3)
        if phys is WALLS:
            assert all(ext[d][s][c] for d in range(3) for s in range(2) for c in range(3)), ext
        if phys is INOUT:
            assert all(ext[0][0]) and not any(ext[0][1]) and all(ext[2][s][c] for s in range(2) for c in range(3))
            assert all(ext[1][s][c] == (c == 1) for s in range(2) for c in range(3)), ext
        if phys is PERIODIC:
            assert not any(ext[d][s][c] for d in range(3) for s in range(2) for c in range(3))
    finally:
        H.close()


@pytest.mark.parametrize("phys", [WALLS, INOUT, PERIODIC], ids=["walls", "inout", "periodic"])
def test_sampling_dm2(gpu, phys):
    pkg = _pkg()
    H = Hier(pkg, 16, [[((0, 0, 0), (7, 15, 0)), ((8, 0, 0), (15, 15, 0))]], phys=phys[:2], nscal=4, dm=2, seed=2, plant_zeros=False)
    try:
        check_sampling(pkg, H, "16^2")
    finally:
        H.close()
        pkg.boxlib.initialize(pkg.capi.default_params())      # (back to dm = 3 for whoever comes next in this process)


@pytest.mark.parametrize("case", ["amr2", "amr3", "odd"])
def test_sampling_hierarchies(gpu, case):
    pkg = _pkg()
    nbase, boxes = ODD if case == "odd" else CASES[case]
    for phys in (WALLS, INOUT):
        H = Hier(pkg, nbase, boxes, phys=phys, nscal=4, seed=4, plant_zeros=False)
        try:
            G = Grid.of(H)
            census = check_sampling(pkg, H, case)
            # every point reports the FINEST level covering it: against a search over all boxes of all levels
            x = lattice_points(G, 2053, 9)
            _, lev = pkg.advance.sample_points(H.mla, H.u, x, H.dx, H.bct, comp=0, nc=1)
            for t in range(0, x.shape[0], 7):
                finest = -1
                for l in range(H.nlev):
                    c = [min(int(np.floor(x[t, d] / H.dx[l][d])), H.n[l][d] - 1) for d in range(3)]
                    if any(all(lo[d] <= c[d] <= hi[d] for d in range(3)) for lo, hi in H.boxes[l]):
                        finest = l
                assert lev[t] == finest, (case, t, x[t], lev[t], finest)
            assert len(census) == H.nlev
        finally:
            H.close()


def test_linear_field(gpu):
    """u = a + B x on amr3, ghost cells included, no face values (periodic types): the interpolation is exact up to the rounding of seven lerps"""
    pkg = _pkg()
    bl = pkg.boxlib
    nbase, boxes = CASES["amr3"]
    H = Hier(pkg, nbase, boxes, phys=PERIODIC, nscal=2, seed=5, plant_zeros=False)
    try:
        a = np.array([0.3, -1.1, 0.7])
        B = np.array([[1.5, -0.4, 0.9], [0.2, 2.1, -1.3], [-0.8, 0.6, 1.7]])
        lin = [bl.MultiFab(H.mla, l, 3, 1) for l in range(H.nlev)]
        for l in range(H.nlev):
            for i in range(lin[l].nfabs()):
                lo, hi = lin[l].get_box(i)
                ax = [(np.arange(lo[d] - 1, hi[d] + 2) + 0.5) * H.dx[l][d] for d in range(3)]
                X, Y, Z = np.meshgrid(*ax, indexing="ij")
                f = np.stack([a[c] + B[c, 0] * X + B[c, 1] * Y + B[c, 2] * Z for c in range(3)], axis=-1)
                lin[l].from_numpy(np.asfortranarray(f), i)
        G = Grid.of(H)
        x = lattice_points(G, 4099, 6)
        val, lev = pkg.advance.sample_points(H.mla, lin, x, H.dx, H.bct, comp=0, nc=3)
        exact = a[None, :] + x @ B.T
        corners = np.array([[(-H.dx[0][d], G.len[d] + H.dx[0][d])[(q >> d) & 1] for d in range(3)] for q in range(8)])
        scale = np.abs(a[None, :] + corners @ B.T).max()                 # max |u| of the field, ghost cells included (a linear function: at a corner)
        err = np.abs(val - exact).max()
        print("linear field on amr3: max error %.3e, bound %.3e, points per level %s" % (err, 16 * 2.0 ** -53 * scale, [int((lev == l).sum()) for l in range(3)]))
        assert err <= 16 * 2.0 ** -53 * scale
        assert all((lev == l).any() for l in range(3))
        for m in lin:
            m.destroy()
    finally:
        H.close()


def test_move_bits(gpu):
    """eight moves on amr2 between two different random velocity fields, 1021 particles: positions and states equal numpy's Heun bit for bit; a second run repeats them"""
    pkg = _pkg()
    nbase, boxes = CASES["amr2"]
    for phys in (WALLS, INOUT):
        H = Hier(pkg, nbase, boxes, phys=phys, nscal=2, seed=6, plant_zeros=False)
        try:
            G = Grid.of(H)
            u1 = second_velocity(pkg, H)
            f0, f1, ext = box_arrays(G, H.u), box_arrays(G, u1), extdir_of(H.bct, 3, 0, 3)
            x0 = lattice_points(G, 1021, 8)
            dt = 0.9 * min(H.dx[0])          # |u| < 1: less than a coarse cell per move, several fine ones
            runs = []
            for rep in range(2):
                P = pkg.advance.Particles(x0)
                assert P.n == 1021 and P.active == 1021
                xr, sr = x0.copy(), np.zeros(1021, dtype=np.int32)
                for k in range(8):
                    P.advance(H.mla, H.u, u1, H.dx, H.bct, dt)
                    if rep == 0:
                        xr, sr = heun(G, f0, f1, ext, xr, sr, dt)
                        x, s = P.positions(), P.state()
                        bad = np.nonzero((u64(x) != u64(xr)).any(axis=1) | (s != sr))[0]
                        assert bad.size == 0, (phys, k, bad[:8], x[bad[:4]], xr[bad[:4]], s[bad[:4]], sr[bad[:4]])
                        assert P.active == int((sr == 0).sum())
                runs.append((u64(P.positions()).copy(), P.state().copy()))
                P.destroy()
            assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
            assert not np.array_equal(runs[0][0], u64(x0))
            if phys is INOUT:
                print("amr2, inflow / outflow: %d of 1021 particles left in 8 moves" % int((runs[0][1] == 1).sum()))
            for m in u1:
                m.destroy()
        finally:
            H.close()


def _uniform_hier(pkg, n, boxes, phys, vel):
    """one level with a velocity given cell by cell by vel(X, Y, Z) -> (u, v, w), ghost cells included"""
    bl = pkg.boxlib
    H = Hier(pkg, n, [boxes], phys=phys, nscal=2, seed=0, plant_zeros=False)
    H.dx = [[1.0 / n] * 3]
    u = bl.MultiFab(H.mla, 0, 3, 1)
    for i in range(u.nfabs()):
        lo, hi = u.get_box(i)
        ax = [(np.arange(lo[d] - 1, hi[d] + 2) + 0.5) * H.dx[0][d] for d in range(3)]
        X, Y, Z = np.meshgrid(*ax, indexing="ij")
        u.from_numpy(np.asfortranarray(np.stack(vel(X, Y, Z), axis=-1)), i)
    return H, [u]


@pytest.mark.parametrize("npart", [1, 63, 4099])
def test_move_uniform_periodic(gpu, npart):
    """a uniform velocity on a periodic 8^3 in two boxes: x_k = (x0 + k dt u) mod L within k 8 2^-53 L, after several wraps"""
    pkg = _pkg()
    uvw = (0.83, -0.41, 0.57)
    H, u = _uniform_hier(pkg, 8, [((0, 0, 0), (3, 7, 7)), ((4, 0, 0), (7, 7, 7))], PERIODIC, lambda X, Y, Z: tuple(np.full(X.shape, c) for c in uvw))
    try:
        G = Grid.of(H)
        x0 = lattice_points(G, npart, 10)
        P = pkg.advance.Particles(x0)
        dt, K = 0.11, 40                     # 3.6 domain lengths along x
        for _ in range(K):
            P.advance(H.mla, u, u, H.dx, H.bct, dt)
        x = P.positions()
        want = np.mod(x0 + K * dt * np.array(uvw)[None, :], 1.0)
        d = np.abs(x - want)
        d = np.minimum(d, 1.0 - d)           # (a particle within rounding of a face may sit on either side of the wrap)
        print("uniform periodic, %d particles, %d moves: max distance %.3e, bound %.3e" % (npart, K, d.max(), K * 8 * 2.0 ** -53))
        assert d.max() <= K * 8 * 2.0 ** -53
        assert P.active == npart and (x >= 0.0).all() and (x <= 1.0).all()
        P.destroy()
        u[0].destroy()
    finally:
        H.close()


@pytest.mark.parametrize("npart", [1, 63, 4099])
def test_move_rigid_rotation(gpu, npart):
    """u = omega x (r - c), linear and steady, on 16^3: the interpolation is exact, so every move is Heun's map of the linear field -- against numpy's Heun of the exact
    field to k 64 2^-53, and the radius grows by Heun's factor sqrt(1 + (omega dt)^4 / 4) per move"""
    pkg = _pkg()
    om = 1.3
    H, u = _uniform_hier(pkg, 16, [((0, 0, 0), (7, 15, 15)), ((8, 0, 0), (15, 15, 15))], WALLS, lambda X, Y, Z: (-om * (Y - 0.5), om * (X - 0.5), np.zeros(X.shape)))
    try:
        rng = np.random.default_rng(12)
        x0 = np.full((npart, 3), 0.5)
        r0 = rng.uniform(0.05, 0.3, npart)
        ph = rng.uniform(0.0, 2 * np.pi, npart)
        x0[:, 0] += r0 * np.cos(ph)
        x0[:, 1] += r0 * np.sin(ph)
        x0[:, 2] = rng.uniform(0.1, 0.9, npart)
        P = pkg.advance.Particles(x0)
        dt, K = 0.05, 12
        xr = x0.copy()
        for k in range(K):
            P.advance(H.mla, u, u, H.dx, H.bct, dt)
            k1 = np.stack([-om * (xr[:, 1] - 0.5), om * (xr[:, 0] - 0.5)], axis=1)
            xs = xr[:, :2] + dt * k1
            k2 = np.stack([-om * (xs[:, 1] - 0.5), om * (xs[:, 0] - 0.5)], axis=1)
            xr[:, :2] = xr[:, :2] + (0.5 * dt) * (k1 + k2)
        x = P.positions()
        err = np.abs(x - xr).max()
        print("rigid rotation, %d particles, %d moves: max |x - numpy Heun| %.3e, bound %.3e" % (npart, K, err, K * 64 * 2.0 ** -53))
        assert err <= K * 64 * 2.0 ** -53
        r = np.hypot(x[:, 0] - 0.5, x[:, 1] - 0.5)
        growth = np.sqrt(1.0 + (om * dt) ** 4 / 4.0) ** K
        assert np.abs(r / r0 - growth).max() <= 2 * K * 64 * 2.0 ** -53 / r0.min()      # (the device against numpy's Heun, numpy's Heun against the factor)
        assert np.array_equal(u64(x[:, 2]), u64(x0[:, 2])) and P.active == npart
        P.destroy()
        u[0].destroy()
    finally:
        H.close()


@pytest.mark.parametrize("npart", [1, 63, 4099])
def test_move_outlet_and_wall(gpu, npart):
    """a uniform flow along +x (into the OUTLET face) and -y (into a wall) on 16^3: a particle gets state 1 at the move whose x' crosses x = 1 and stays where it
    was; at the wall it is mirrored back and stays inside, within one move of the wall"""
    pkg = _pkg()
    uvw = (0.9, -0.7, 0.0)
    H, u = _uniform_hier(pkg, 16, [((0, 0, 0), (7, 15, 15)), ((8, 0, 0), (15, 15, 15))], INOUT, lambda X, Y, Z: tuple(np.full(X.shape, c) for c in uvw))
    try:
        G = Grid.of(H)
        x0 = lattice_points(G, npart, 13)
        P = pkg.advance.Particles(x0)
        f, ext = box_arrays(G, u), extdir_of(H.bct, 3, 0, 3)
        dt, K = 0.07, 14
        xr, sr = x0.copy(), np.zeros(npart, dtype=np.int32)
        gone_at = np.full(npart, -1)
        for k in range(K):
            P.advance(H.mla, u, u, H.dx, H.bct, dt)
            xr, sr = heun(G, f, f, ext, xr, sr, dt)
            gone_at[(sr == 1) & (gone_at < 0)] = k
            assert np.array_equal(P.state(), sr), k
            assert P.active == int((sr == 0).sum())
        x = P.positions()
        assert np.array_equal(u64(x), u64(xr))
        # numpy's prediction of the step a particle leaves at: the first k with x0 + (k + 1) dt u > 1 (up to the rounding of the sum at the face)
        k_exact = np.ceil((1.0 - x0[:, 0]) / (dt * uvw[0]) - 1e-9).astype(int) - 1
        sure = np.abs((1.0 - x0[:, 0]) / (dt * uvw[0]) - np.round((1.0 - x0[:, 0]) / (dt * uvw[0]))) > 1e-6
        left = gone_at >= 0
        assert np.array_equal(left[sure], (k_exact < K)[sure])
        assert np.array_equal(gone_at[left & sure], k_exact[left & sure])
        assert (x[left, 0] <= 1.0).all() and (x[left, 0] > 1.0 - dt * uvw[0] - 1e-12).all()      # frozen at the last position inside
        assert (x[:, 1] >= 0.0).all() and (x[:, 1] <= 1.0).all()
        # at the wall: the flow keeps pushing a particle down and every crossing is mirrored back, so once there it stays within one move of the wall;
        # a particle that has not reached it is on its straight path
        moves = np.where(left, gone_at, K)
        free = x0[:, 1] + moves * dt * uvw[1]
        hit = free < 0.0
        assert (x[hit, 1] <= dt * abs(uvw[1])).all()
        assert np.abs(x[~hit, 1] - free[~hit]).max(initial=0.0) <= K * 8 * 2.0 ** -53
        if npart > 1:
            assert left.any() and (~left).any() and hit.any() and (~hit).any()
        P.destroy()
        u[0].destroy()
    finally:
        H.close()


def test_ranks_give_identical_bits(gpu, tmp_path):
    """amr3, three moves and a sampling, on one, two and four ranks (the RCCL test double): the same bits on every rank and on any number of ranks"""
    out = {}
    keys = ("x", "state", "val", "lev", "active")
    for nranks, per_proc in ((1, 1), (2, 1), (4, 2)):
        out[nranks] = launch_ranks("_particles_worker.py", nranks, tmp_path, "part%d" % nranks, ["amr3"], per_proc=per_proc, agree=keys, timeout=300)
    for nranks in (2, 4):
        for key in keys:
            assert np.array_equal(out[nranks][key], out[1][key]), (nranks, key)
    assert out[1]["active"][0] == 1021 and (out[1]["lev"] >= 0).all() and len(set(out[1]["lev"].tolist())) == 3


def test_varden_fields_unchanged(gpu):
    """Varden 16^3 in two boxes with an 8^3 lattice, three steps: the particles rest during the start-up iterations, move afterwards, and uold, sold, gp, p after the
    run are the bits of the same run without particles (the ghost fill of unew before the move is the one the next step's top repeats)"""
    _pkg()
    from varden_amd import advance as adv
    from varden_amd import driver
    from varden_amd.capi import default_params
    x0 = adv.particle_lattice((8, 8, 8), (1.0, 1.0, 1.0))
    assert x0.shape == (512, 3) and x0[1, 0] - x0[0, 0] == 0.125 and x0[0, 1] == x0[1, 1]
    for swap in (False, True):
        finals = {}
        for with_particles in (True, False):
            S = driver.Varden(16, WALLS, default_params(), init_shrink=0.1, init_iter=1, decomp=(2, 1, 1), swap_state=swap, particles=x0 if with_particles else None)
            if with_particles:
                assert np.array_equal(u64(S.particles.positions()), u64(x0))
            for k in range(3):
                S.step()
            finals[with_particles] = [u64(np.concatenate([m.to_numpy(i).ravel() for i in range(m.nfabs())])) for m in (S.uold[0], S.sold[0], S.gp[0], S.p[0])]
            if with_particles:
                xp = S.particles.positions()
                assert np.isfinite(xp).all() and S.particles.active == 512 and not np.array_equal(u64(xp), u64(x0))
            S.close()
        for a, b, name in zip(finals[True], finals[False], ("uold", "sold", "gp", "p")):
            if swap and name in ("uold", "sold"):      # (after a handle swap the ghost cells of uold are those of the previous unew: the valid cells are the state)
                continue
            assert np.array_equal(a, b), (swap, name)


def test_varden_moves_replayed(gpu):
    """the same run stepped by hand, so that both velocity fields of every move are at hand: the driver's placement (fill unew's ghosts, move, then copy) replayed in
    numpy, bit for bit"""
    pkg = _pkg()
    from varden_amd import advance as adv
    from varden_amd import boxlib as bl
    from varden_amd import driver
    from varden_amd.capi import default_params
    x0 = adv.particle_lattice((8, 8, 8), (1.0, 1.0, 1.0))
    S = driver.Varden(16, WALLS, default_params(), init_shrink=0.1, init_iter=1, decomp=(2, 1, 1), particles=x0)
    T = driver.Varden(16, WALLS, default_params(), init_shrink=0.1, init_iter=1, decomp=(2, 1, 1))      # the same run without particles, one step behind where needed
    try:
        G = Grid([(16, 16, 16)], S.dx, [S.boxes], WALLS)
        ext = extdir_of(S.bct, 3, 0, 3)
        xr, sr = x0.copy(), np.zeros(512, dtype=np.int32)
        for k in range(3):
            # T's step up to the copy: its uold (ghosts filled at the top) and unew (ghosts filled as step() fills them for the move) are the move's two fields
            T.istep += 1
            T.fill_state_ghosts()
            if T.istep > 1:
                T.dt = driver._limit_dt(T, T.estdt(T.dt))
            T.advance(bl.REGULAR_TIMESTEP, T.istep)
            T.unew[0].fill_boundary()
            T.unew[0].physbc(0, 0, 3, T.bct)
            xr, sr = heun(G, box_arrays(G, T.uold), box_arrays(G, T.unew), ext, xr, sr, T.dt)
            T.uold[0].copy_c(0, T.unew[0], 0, 3, 0)
            T.sold[0].copy_c(0, T.snew[0], 0, T.nscal, 0)
            T.time += T.dt
            S.step()
            assert S.dt == T.dt
            bad = np.nonzero((u64(S.particles.positions()) != u64(xr)).any(axis=1))[0]
            assert bad.size == 0, (k, bad[:8])
            assert np.array_equal(S.particles.state(), sr)
        assert np.abs(S.particles.positions() - x0).max() > 0.0
    finally:
        S.close()
        T.close()


def test_amr_run_with_regrids(gpu):
    """VardenAMR, 32^3 base, three levels, regrid_int = 2, six steps with a 6^3 lattice: every particle stays active and finite, the census of host levels changes
    across a regrid, and the fields are the bits of the run without particles"""
    pkg = _pkg()
    from varden_amd import advance as adv
    from varden_amd import driver
    from varden_amd.capi import default_params
    x0 = adv.particle_lattice((6, 6, 6), (1.0, 1.0, 1.0))
    x0 = 0.5 + 0.45 * (x0 - 0.5)                    # around the bubble, where the fine levels are
    finals, census = {}, []
    # the run starts on grids that miss the bubble: the regrid at the top of step 1 moves them onto it
    first = dict(fine_boxes=[((8, 8, 8), (39, 39, 39))], finer_levels=[[((24, 24, 24), (55, 55, 55))]])
    for with_particles in (True, False):
        S = driver.VardenAMR(32, first["fine_boxes"], WALLS, params=default_params(cflfac=0.9), finer_levels=first["finer_levels"], init_shrink=0.1, init_iter=1,
                             do_initial_projection=1, regrid_int=2, max_levs=3, max_grid_size=32, particles=x0 if with_particles else None)
        for k in range(7):
            if with_particles:
                _, lev = S.particles.sample(S.mla, S.sold, S.dx, S.bct, comp=0, nc=S.nscal, bccomp=3, levels=True)
                census.append(tuple(int((lev == l).sum()) for l in range(3)))
            if k < 6:
                S.step()
        finals[with_particles] = [[u64(np.concatenate([m.to_numpy(i).ravel() for i in range(m.nfabs())])) for m in lst] for lst in (S.uold, S.sold, S.gp, S.p)]
        if with_particles:
            xp = S.particles.positions()
            assert np.isfinite(xp).all() and S.particles.active == x0.shape[0]
            assert S.nregrids >= 3
            print("host-level census per step:", census)
            assert all(sum(c) == x0.shape[0] for c in census) and census[0] != census[1]      # before and after the first regrid
            # every reported level is the finest that covers the particle on the CURRENT grids
            G = Grid([tuple(32 << l for _ in range(3)) for l in range(S.nlev)], S.dx, S.boxes, WALLS)
            host, _ = locate(G, xp)
            _, lev = S.particles.sample(S.mla, S.sold, S.dx, S.bct, comp=0, nc=1, bccomp=3, levels=True)
            assert np.array_equal(host, lev)
        S.close()
    for la, lb, name in zip(finals[True], finals[False], ("uold", "sold", "gp", "p")):
        assert len(la) == len(lb), name
        for a, b in zip(la, lb):
            assert np.array_equal(a, b), name


def test_files(gpu, tmp_path):
    """write, read, write: the same bytes; positions, states, time and columns come back; a short file and a foreign one are refused"""
    pkg = _pkg()
    from varden_amd import advance as adv
    from varden_amd import capi
    pkg.boxlib.initialize(capi.default_params())
    rng = np.random.default_rng(20)
    x0 = rng.uniform(0.0, 1.0, (257, 3))
    P = adv.Particles(x0)
    cols = {"u": rng.normal(size=257), "v": rng.normal(size=257), "rho": rng.normal(size=257)}
    a, b = str(tmp_path / "part00001"), str(tmp_path / "again")
    t = 0.1 + 2.0 ** -40
    P.write(a, time=t, columns=cols)
    Q, tq, cq = adv.Particles.read(a)
    assert tq == t and list(cq) == ["u", "v", "rho"] and all(np.array_equal(u64(cq[k]), u64(cols[k])) for k in cols)
    assert Q.n == 257 and np.array_equal(u64(Q.positions()), u64(x0)) and (Q.state() == 0).all()
    Q.write(b, time=tq, columns=cq)
    raw = open(a, "rb").read()
    assert raw == open(b, "rb").read()
    assert raw.startswith(b"VDN_PARTICLES 1\ndm 3\nn 257\nncol 3\nu\nv\nrho\ntime ")
    assert len(raw) == raw.index(b"\n", raw.index(b"time ")) + 1 + 257 * (4 + 24 + 3 * 8)
    # no columns at all
    P.write(b, time=0.0)
    R, tr, cr = adv.Particles.read(b)
    assert tr == 0.0 and cr == {} and np.array_equal(u64(R.positions()), u64(x0))
    # refusals: a file cut inside the positions, inside the columns, a foreign first line, a missing file
    for cut, word in ((raw.index(b"time ") + 40 + 257 * 4 + 100, "short"), (len(raw) - 8, "short")):
        open(b, "wb").write(raw[:cut])
        with pytest.raises(capi.VardenError, match=word):
            adv.Particles.read(b)
    open(b, "wb").write(b"VDN_PARTICLE5 1\n" + raw[16:])
    with pytest.raises(capi.VardenError, match="not a particle file"):
        adv.Particles.read(b)
    with pytest.raises(capi.VardenError, match="cannot open"):
        adv.Particles.read(str(tmp_path / "nothing"))
    for p in (P, Q, R):
        p.destroy()


def test_refusals(gpu):
    """every refusal of include/varden_amd.h, and a good call afterwards"""
    import ctypes as C
    pkg = _pkg()
    from varden_amd import advance as adv
    from varden_amd import boxlib as bl
    from varden_amd import capi
    from varden_amd.boxlib import handle_array
    lib = capi.load()
    nbase, boxes = CASES["amr2"]
    H = Hier(pkg, nbase, boxes, nscal=2, seed=7, plant_zeros=False)
    try:
        G = Grid.of(H)
        x = lattice_points(G, 33, 1)
        dx = adv._dx3(H.dx)
        xp, val, lev = x.ctypes.data_as(C.POINTER(C.c_double)), np.zeros((33, 3)), np.zeros(33, dtype=np.int32)
        vp, lp = val.ctypes.data_as(C.POINTER(C.c_double)), lev.ctypes.data_as(C.POINTER(C.c_int))
        P = adv.Particles(x)
        nodal = [bl.MultiFab(H.mla, l, 3, 1, (1, 1, 1)) for l in range(2)]
        noghost = [bl.MultiFab(H.mla, l, 3, 0) for l in range(2)]
        other = Hier(pkg, nbase, boxes, nscal=2, seed=8, plant_zeros=False)
        u, mla, bct = handle_array(H.u), H.mla.h, H.bct.h

        def refused(rc, word):
            assert rc != 0, word
            msg = lib.vdn_last_error().decode()
            assert word in msg, (word, msg)

        refused(lib.vdn_sample_points(2, None, u, 0, 3, 0, dx, bct, 33, xp, vp, lp), "null")
        refused(lib.vdn_sample_points(2, mla, None, 0, 3, 0, dx, bct, 33, xp, vp, lp), "null")
        refused(lib.vdn_sample_points(2, mla, u, 0, 3, 0, dx, bct, 33, None, vp, lp), "null")
        refused(lib.vdn_sample_points(2, mla, u, 0, 3, 0, dx, bct, 33, xp, None, lp), "null")
        refused(lib.vdn_sample_points(1, mla, u, 0, 3, 0, dx, bct, 33, xp, vp, lp), "does not match the layout")
        refused(lib.vdn_sample_points(2, mla, handle_array(other.u), 0, 3, 0, dx, bct, 33, xp, vp, lp), "not a multifab of level")
        refused(lib.vdn_sample_points(2, mla, handle_array(nodal), 0, 3, 0, dx, bct, 33, xp, vp, lp), "nodal")
        refused(lib.vdn_sample_points(2, mla, u, 1, 3, 0, dx, bct, 33, xp, vp, lp), "components")
        refused(lib.vdn_sample_points(2, mla, handle_array(noghost), 0, 3, 0, dx, bct, 33, xp, vp, lp), "ghost")
        refused(lib.vdn_sample_points(2, mla, u, 0, 3, 0, dx, None, 33, xp, vp, lp), "bct is NULL")
        refused(lib.vdn_sample_points(2, mla, u, 0, 3, 0, None, bct, 33, xp, vp, lp), "dx is NULL")
        refused(lib.vdn_sample_points(2, mla, u, 0, 3, 0, dx, bct, 0, xp, vp, lp), "at least 1")
        refused(lib.vdn_particles_create(0, xp, C.byref(C.c_void_p())), "at least 1")
        refused(lib.vdn_particles_create(33, None, C.byref(C.c_void_p())), "null")
        refused(lib.vdn_particles_create(33, xp, None), "null")
        bad = x.copy()
        bad[5, 1] = np.nan
        refused(lib.vdn_particles_create(33, bad.ctypes.data_as(C.POINTER(C.c_double)), C.byref(C.c_void_p())), "not finite")
        bad[5, 1] = 2.5 * G.len[1]
        Q = adv.Particles(bad)                      # the domain is known at the first call that names the hierarchy
        refused(lib.vdn_particles_advance(Q.h, 2, mla, u, u, dx, bct, 0.01), "outside the domain")
        refused(lib.vdn_particles_sample(Q.h, 2, mla, u, 0, 3, 0, dx, bct, vp, lp), "outside the domain")
        Q.destroy()
        refused(lib.vdn_particles_advance(None, 2, mla, u, u, dx, bct, 0.01), "null")
        refused(lib.vdn_particles_advance(P.h, 2, mla, u, None, dx, bct, 0.01), "null")
        refused(lib.vdn_particles_advance(P.h, 1, mla, u, u, dx, bct, 0.01), "does not match the layout")
        refused(lib.vdn_particles_advance(P.h, 2, mla, u, handle_array(noghost), dx, bct, 0.01), "ghost")
        refused(lib.vdn_particles_advance(P.h, 2, mla, handle_array(H.s), u, dx, bct, 0.01), "components")
        refused(lib.vdn_particles_advance(P.h, 2, mla, u, u, dx, None, 0.01), "bct is NULL")
        refused(lib.vdn_particles_advance(P.h, 2, mla, u, u, None, bct, 0.01), "dx is NULL")
        refused(lib.vdn_particles_sample(None, 2, mla, u, 0, 3, 0, dx, bct, vp, lp), "null")
        refused(lib.vdn_particles_sample(P.h, 2, mla, u, 0, 3, 0, dx, bct, None, lp), "null")
        refused(lib.vdn_particles_get(None, xp, lp), "null")
        refused(lib.vdn_particles_count(None, None, None), "null")
        refused(lib.vdn_particles_write(P.h, None, 0.0, 0, None, None), "null")
        refused(lib.vdn_particles_write(P.h, b"/nonexistent-dir/part", 0.0, 0, None, None), "cannot open")
        refused(lib.vdn_particles_read(None, C.byref(C.c_void_p()), None), "null")
        # nothing of all that is left in the arena, and the library still runs good calls
        val2, lev2 = adv.sample_points(H.mla, H.u, x, H.dx, H.bct, comp=0, nc=3)
        ref, rlev = sample(G, box_arrays(G, H.u), extdir_of(H.bct, 3, 0, 3), x, 3)
        assert np.array_equal(u64(val2), u64(ref)) and np.array_equal(lev2, rlev)
        P.advance(H.mla, H.u, H.u, H.dx, H.bct, 0.01)
        assert P.active == 33
        P.destroy()
        for m in nodal + noghost:
            m.destroy()
        other.close()
    finally:
        H.close()


def test_refuses_dm2_hierarchy_and_locator_cap(gpu):
    """dm = 2 with two levels, and a level whose block map would exceed 2^25 entries (a 512^3 level with a box aligned to nothing), are refused by name"""
    pkg = _pkg()
    from varden_amd import advance as adv
    from varden_amd import boxlib as bl
    from varden_amd import capi
    bl.initialize(capi.default_params())
    pd = [((0, 0, 0), (255, 255, 255)), ((0, 0, 0), (511, 511, 511))]
    mla = bl.MLLayout(pd, [[pd[0]], [((1, 1, 1), (6, 6, 6))]], rr=[(2, 2, 2)])
    bct = bl.BCTower(mla, WALLS)
    # multifabs of one cell's worth would do, but a multifab covers its level: the 256^3 base with one component is 134 MB, allocated and freed here
    mfs = [bl.MultiFab(mla, 0, 1, 1), bl.MultiFab(mla, 1, 1, 1)]
    try:
        with pytest.raises(capi.VardenError, match=r"level 1.*1 x 1 x 1"):
            adv.sample_points(mla, mfs, np.array([[0.5, 0.5, 0.5]]), [[1.0 / 256] * 3, [1.0 / 512] * 3], bct, comp=0, nc=1)
    finally:
        for m in mfs:
            m.destroy()
        bct.destroy()
        mla.destroy()
    H = Hier(pkg, 16, [[((0, 0, 0), (15, 15, 0))]], phys=WALLS[:2], nscal=2, dm=2, seed=2, plant_zeros=False)
    try:
        import ctypes as C
        two = bl.MLLayout([((0, 0, 0), (15, 15, 0)), ((0, 0, 0), (31, 31, 0))], [[((0, 0, 0), (15, 15, 0))], [((8, 8, 0), (23, 23, 0))]], rr=[(2, 2, 1)])
        tower = bl.BCTower(two, [[15, 15], [15, 15], [0, 0]])
        u2 = [bl.MultiFab(two, l, 2, 1) for l in range(2)]
        x = np.array([[0.5, 0.5, 0.0]])
        val, lev = np.zeros((1, 2)), np.zeros(1, dtype=np.int32)
        rc = capi.load().vdn_sample_points(2, two.h, bl.handle_array(u2), 0, 2, 0, adv._dx3([H.dx[0], [0.5 * v for v in H.dx[0]]]), tower.h, 1,
                                           x.ctypes.data_as(C.POINTER(C.c_double)), val.ctypes.data_as(C.POINTER(C.c_double)), lev.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc != 0
        msg = capi.load().vdn_last_error().decode()
        assert "dm = 2 runs on one level" in msg, msg
        for m in u2:
            m.destroy()
        tower.destroy()
        two.destroy()
    finally:
        H.close()
        bl.initialize(capi.default_params())
