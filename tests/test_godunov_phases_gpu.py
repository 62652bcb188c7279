"""The fused Godunov marches of a one-box level run each k-chunk in phases -- warm-up planes, steady planes with every start-up condition compiled in,
run-out planes -- and, on power-of-two spacings, with the launch's flags (cons, use_minion, the update's forcing mode) as template arguments.  Neither
changes a value: the default launch forms against the face-centred one-thread-per-cell kernels, SHA-256 over the valid cells / faces, for chunk lengths
1, 2, 3 (no steady plane), 4 (one) and >= 6, on boxes with a narrow remainder column (kk_vp_F_mc / kk_mk_F_mc) and boxes narrower than a tile
(kk_vp_F_m / kk_mk_F_m), under walls, the four-rule mix and full periodicity, with use_minion 0 and 1.  The switches are read at a process's first
launch, hence the child processes."""
import math
import textwrap

import pytest

from tests.children import ROOT, line, run_variant

pytestmark = pytest.mark.gpu

FNX, TNY = 62, 8
FNY = TNY - 2
PLAIN = {"VDN_GODUNOV_PLAIN": "1", "VDN_SLOPES_MARCH": "0"}


def _best_klen(tiles, nz):
    """the chunk length fused_grid / fused_grid_cols choose (godunov.hip): the chunk count with the least rounds x iterations per workgroup"""
    best, best_cost = 1, 1e300
    for ch in range(1, min(16, nz) + 1):
        kl = (nz + ch - 1) // ch
        nch = (nz + kl - 1) // kl
        cost = math.ceil(tiles * nch / 256.0) * (kl + 4)
        if cost < best_cost:
            best, best_cost = ch, cost
    return (nz + best - 1) // best


def klen_cols(nx, ny, nz):
    """fused_grid_cols on the face range of an nx x ny x nz box (one face more per direction); None where the box has no narrow remainder column"""
    nx, ny, nz = nx + 1, ny + 1, nz + 1
    full, rem = nx // FNX, nx % FNX
    if full < 1 or rem <= 0 or rem + 2 > 32:
        return None
    rows = TNY * (64 // (rem + 2)) - 2
    return _best_klen(full * ((ny + FNY - 1) // FNY) + (ny + rows - 1) // rows, nz)


def klen_tiles(nx, ny, nz, chunks=0):
    """fused_grid on the same range; chunks: VDN_FUSED_KCHUNKS"""
    nx, ny, nz = nx + 1, ny + 1, nz + 1
    if chunks:
        return max(1, (nz + chunks - 1) // chunks)
    return _best_klen(((nx + FNX - 1) // FNX) * ((ny + FNY - 1) // FNY), nz)


BCS = {"walls": [[15, 15]] * 3, "mix": [[11, 12], [14, 15], [15, 12]], "periodic": [[-1, -1]] * 3}

KERNEL_CODE = textwrap.dedent("""
    import sys, hashlib
    sys.path.insert(0, %r)
    import numpy as np
    from varden_amd import advance as adv, boxlib as bl, capi
    nx, ny, nz, minion = (int(a) for a in sys.argv[1:5])
    phys = [[int(a) for a in sys.argv[5 + 2 * d:7 + 2 * d]] for d in range(3)]
    bl.initialize(capi.default_params(use_minion=minion), 0, 1, 0)
    lo, hi = (0, 0, 0), (nx - 1, ny - 1, nz - 1)
    pmask = tuple(1 if phys[d][0] == bl.PERIODIC else 0 for d in range(3))
    mla = bl.MLLayout([(lo, hi)], [[(lo, hi)]], pmask=pmask)
    bct = bl.BCTower(mla, phys)
    rng = np.random.default_rng(11)
    def mf(nc, ng, nodal=None):
        m = bl.MultiFab(mla, 0, nc, ng, nodal)
        m.from_numpy(rng.standard_normal(m.shape(0))); return m
    def valid(m):
        a, g = m.to_numpy(), m.ng
        return a[g:a.shape[0] - g, g:a.shape[1] - g, g:a.shape[2] - g]
    u, s = mf(3, 3), mf(2, 3)
    f3, f2, rhs = mf(3, 1), mf(2, 1), mf(1, 1)
    nd = [tuple(1 if t == d else 0 for t in range(3)) for d in range(3)]
    umac = [mf(1, 1, nd[d]) for d in range(3)]
    ue = [mf(3, 0, nd[d]) for d in range(3)]; uf = [mf(3, 0, nd[d]) for d in range(3)]
    se = [mf(2, 0, nd[d]) for d in range(3)]; sf = [mf(2, 0, nd[d]) for d in range(3)]
    dx, dt = [1.0 / 64] * 3, 0.3 / 64                     # powers of two: the marches that scale by 1 / dx, flags compiled in
    adv.velpred(u, umac, f3, dx, dt, bct)
    for m in umac: m.fill_boundary()
    adv.mkflux(u, ue, uf, umac, f3, rhs, dx, dt, bct, True, [0, 0, 0])
    adv.mkflux(s, se, sf, umac, f2, rhs, dx, dt, bct, False, [1, 0])
    h = hashlib.sha256()
    for m in umac + ue + se + [sf[d] for d in range(3)]:
        h.update(np.ascontiguousarray(valid(m)).tobytes())
    print("HASH", h.hexdigest())
""" % ROOT)


def _phys_args(bc):
    return tuple(v for d in range(3) for v in BCS[bc][d])


# a box with a narrow remainder column (62 + 10 cells; velpred takes kk_vp_F_mc, mkflux without the update kk_mk_F_m in two tile columns), three tile rows;
# nz chosen for the chunk length of the column launch
COL_SHAPES = {1: (72, 14, 15), 2: (72, 14, 19), 3: (72, 14, 34), 4: (72, 14, 49), 6: (72, 14, 82)}


@pytest.mark.parametrize("minion", [0, 1])
@pytest.mark.parametrize("bc", list(BCS))
@pytest.mark.parametrize("klen", list(COL_SHAPES))
def test_marches_with_remainder_column_equal_face_centred(gpu, klen, bc, minion):
    n = COL_SHAPES[klen]
    assert klen_cols(*n) == klen, "the chunk rule no longer gives klen %d on %r: %r" % (klen, n, klen_cols(*n))
    args = n + (minion,) + _phys_args(bc)
    out = [line(run_variant(("-c", KERNEL_CODE) + args, sw, 300), "HASH") for sw in ({}, PLAIN)]
    assert out[0] == out[1], (n, bc, minion, klen_tiles(*n), out)


# a box narrower than a tile (kk_vp_F_m / kk_mk_F_m), three tile rows, 12 planes of cells = 13 of faces: VDN_FUSED_KCHUNKS sets the chunk count
NARROW_SHAPE = (24, 14, 12)
CHUNKS = {1: 13, 2: 7, 3: 5, 4: 4, 7: 2}


@pytest.mark.parametrize("minion", [0, 1])
@pytest.mark.parametrize("bc", list(BCS))
def test_marches_narrower_than_a_tile_equal_face_centred(gpu, bc, minion):
    n = NARROW_SHAPE
    assert klen_cols(*n) is None
    for klen, ch in CHUNKS.items():
        assert klen_tiles(*n, chunks=ch) == klen, (klen, ch, klen_tiles(*n, chunks=ch))
    args = n + (minion,) + _phys_args(bc)
    ref = line(run_variant(("-c", KERNEL_CODE) + args, PLAIN, 300), "HASH")
    for klen, ch in CHUNKS.items():
        got = line(run_variant(("-c", KERNEL_CODE) + args, {"VDN_FUSED_KCHUNKS": str(ch)}, 300), "HASH")
        assert got == ref, (n, bc, minion, klen, got, ref)


STEP_CODE = textwrap.dedent("""
    import sys, hashlib
    sys.path.insert(0, %r)
    import numpy as np
    from varden_amd import driver
    from varden_amd.capi import default_params
    nx, ny, nz, minion = (int(a) for a in sys.argv[1:5])
    # every spacing 1 / 64: the update-carrying marches with cons / use_minion / the forcing mode compiled in (velocity: cons 0, forcing formed in
    # place; density: cons 1; tracer: cons 0, the force of the call)
    G = driver.Varden((nx, ny, nz), [[15, 15]] * 3, default_params(use_minion=minion), prob_hi=(nx / 64.0, ny / 64.0, nz / 64.0), init_iter=1)
    for _ in range(2):
        G.step()
        h = hashlib.sha256()
        for m in (G.unew[0], G.snew[0], G.gp[0]):
            h.update(np.ascontiguousarray(G.gather_valid(m)).tobytes())
        print("HASH", h.hexdigest())
    G.close()
""" % ROOT)
STEP_REF = {"VDN_GOD_UPDATE": "0", "VDN_GODUNOV_PLAIN": "1", "VDN_NO_FORCE_REUSE": "1"}
# remainder column (kk_mk_F_mc + update), sizes the multigrids accept; then a box narrower than a tile (kk_mk_F_m + update) under VDN_FUSED_KCHUNKS
STEP_SHAPES = {1: (72, 16, 12), 2: (72, 16, 24), 3: (72, 16, 40), 4: (72, 16, 56), 6: (72, 16, 88)}


def _step_hashes(args, sw):
    r = run_variant(("-c", STEP_CODE) + args, sw, 300)
    return [" ".join(t) for t in r["HASH"]]


@pytest.mark.parametrize("minion", [0, 1])
@pytest.mark.parametrize("klen", list(STEP_SHAPES))
def test_steps_with_remainder_column_equal_separate_update(gpu, klen, minion):
    n = STEP_SHAPES[klen]
    assert klen_cols(*n) == klen, "the chunk rule no longer gives klen %d on %r: %r" % (klen, n, klen_cols(*n))
    out = [_step_hashes(n + (minion,), sw) for sw in ({}, STEP_REF)]
    assert len(out[0]) == 2 and out[0] == out[1], (n, minion, out)


@pytest.mark.parametrize("minion", [0, 1])
def test_steps_narrower_than_a_tile_equal_separate_update(gpu, minion):
    n = (24, 16, 12)
    ref = _step_hashes(n + (minion,), STEP_REF)
    assert len(ref) == 2
    for klen, ch in ((1, 13), (3, 5), (4, 4), (7, 2)):
        assert klen_tiles(*n, chunks=ch) == klen
        got = _step_hashes(n + (minion,), {"VDN_FUSED_KCHUNKS": str(ch)})
        assert got == ref, (n, minion, klen, got, ref)
